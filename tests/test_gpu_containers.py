"""GPU: the device-side containers (`next` binary heap, `top` sorted buffer) against a literal Python restatement of the
reference containers (max_heap_gt index.hpp:664-835, sorted_buffer_gt index.hpp:845-956) on tie-heavy scripts."""
import numpy as np
import pytest

from tests.container_model import RefHeap

pytestmark = pytest.mark.gpu


def ref_sorted_insert(buf, d, slot, limit):
    lo = 0
    while lo < len(buf) and buf[lo][0] < d:
        lo += 1
    if lo == limit:
        return
    if len(buf) == limit:
        buf.pop()
    buf.insert(lo, (d, slot))


@pytest.mark.parametrize("seed,levels,count,limit", [(0, 4, 300, 16), (1, 1000, 500, 64), (2, 2, 700, 100),
                                                     (3, 8, 64, 1), (4, 3, 1000, 200)])
def test_containers_match_reference_rules(seed, levels, count, limit):
    from usearch_amd import index as ua
    rng = np.random.default_rng(seed)
    kinds = rng.choice([0, 0, 0, 1, 2, 2], size=count).astype(np.uint32)
    keys = rng.integers(0, levels, size=count).astype(np.float32) * 0.5 - 1.0  # few distinct values ⇒ ties everywhere
    slots = np.arange(count, dtype=np.uint32)
    heap, top, popped = RefHeap(), [], []
    for kind, key, slot in zip(kinds, keys, slots):
        if kind == 0:
            heap.push(float(key), int(slot))
        elif kind == 1 and heap.e:
            popped.append(heap.pop())
        elif kind == 2:
            ref_sorted_insert(top, float(key), int(slot), limit)
    (pk, ps), (tk, ts) = ua.test_containers(kinds, keys, slots, limit)
    assert [(float(a), int(b)) for a, b in zip(pk, ps)] == popped
    assert [(float(a), int(b)) for a, b in zip(tk, ts)] == top


@pytest.mark.parametrize("global_memory", [False, True])
@pytest.mark.parametrize("form", ["distinct", "eight levels", "5% nan"])
def test_deep_heap_matches_reference_rules(form, global_memory):
    """2 600 pushes, then 1 500 pop / push pairs, in LDS and in device memory (`global_ak = true`): what is popped, then what remains,
    cell by cell, equals `max_heap_gt`. The heap's rules are comparisons in a fixed order, which have a definite answer for NaN too, so
    the 5 % NaN form is held to the same reference. `heap_pop` settles five levels per round: its third round needs more than 2 047
    entries below the root, which the walks' frontiers reach only on filtered searches at large expansions."""
    from usearch_amd import index as ua
    rng = np.random.default_rng(11)
    fill, pairs = 2600, 1500
    count = fill + 2 * pairs
    kinds = np.zeros(count, dtype=np.uint32)
    kinds[fill::2] = 1
    if form == "distinct":
        keys = rng.permutation(count).astype(np.float32) * -0.125
    else:
        keys = rng.integers(0, 8, size=count).astype(np.float32) * -0.5
        if form == "5% nan":
            keys[rng.random(count) < 0.05] = np.nan
    slots = np.arange(count, dtype=np.uint32)
    heap, popped, deepest = RefHeap(), [], 0
    for kind, key, slot in zip(kinds, keys, slots):
        if kind == 0:
            heap.push(float(key), int(slot))
        else:
            deepest = max(deepest, len(heap.e))
            popped.append(heap.pop())
    assert deepest > 2047 and len(popped) == pairs, "the script must reach the third round of `heap_pop`"
    (pk, ps), (tk, ts), (hk, hs) = ua.test_containers(kinds, keys, slots, 1, global_memory=global_memory, remains=True)
    bits = keys.view(np.uint32)
    assert ps.tolist() == [slot for _, slot in popped]
    assert pk.view(np.uint32).tolist() == [int(bits[slot]) for _, slot in popped]
    assert hs.tolist() == [slot for _, slot in heap.e]
    assert hk.view(np.uint32).tolist() == [int(bits[slot]) for _, slot in heap.e]
    assert len(tk) == 0 and len(ts) == 0


@pytest.mark.parametrize("seed,levels,count,limit", [(0, 4, 300, 16), (3, 8, 64, 1), (4, 3, 1000, 200)])
def test_containers_in_device_memory_match_reference_rules(seed, levels, count, limit):
    """The scripts of `test_containers_match_reference_rules` on the `global_ak = true` variants of the same containers."""
    from usearch_amd import index as ua
    rng = np.random.default_rng(seed)
    kinds = rng.choice([0, 0, 0, 1, 2, 2], size=count).astype(np.uint32)
    keys = rng.integers(0, levels, size=count).astype(np.float32) * 0.5 - 1.0
    slots = np.arange(count, dtype=np.uint32)
    heap, top, popped = RefHeap(), [], []
    for kind, key, slot in zip(kinds, keys, slots):
        if kind == 0:
            heap.push(float(key), int(slot))
        elif kind == 1 and heap.e:
            popped.append(heap.pop())
        elif kind == 2:
            ref_sorted_insert(top, float(key), int(slot), limit)
    (pk, ps), (tk, ts), (hk, hs) = ua.test_containers(kinds, keys, slots, limit, global_memory=True, remains=True)
    assert [(float(a), int(b)) for a, b in zip(pk, ps)] == popped
    assert [(float(a), int(b)) for a, b in zip(tk, ts)] == top
    assert [(float(a), int(b)) for a, b in zip(hk, hs)] == heap.e


def micro_benchmarks(waves=3, fill=32, count=64, limit=16):
    """What the two diagnostic hooks of csrc/test_hooks.hip report that does not depend on the clock: per wave, the checksum of what
    the heap popped (serial and subtree pop) and how many candidates `top` accepted (4, 8 and 16 entries per lane)."""
    import ctypes as C

    from usearch_amd import index as ua
    hooks = ua.test_hooks()
    hooks.usearch_amd_bench_heap.argtypes = [C.c_uint32] * 4 + [C.c_void_p] * 3 + [C.POINTER(C.c_char_p)]
    hooks.usearch_amd_bench_top.argtypes = [C.c_uint32] * 4 + [C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p)]
    checksums, ticks, accepted = {}, {}, {}
    for serial in (1, 0):
        pops, pushes, checksums[serial] = (np.zeros(waves, dtype=np.uint64) for _ in range(3))
        err = C.c_char_p()
        hooks.usearch_amd_bench_heap(serial, fill, count, waves, pops.ctypes.data, pushes.ctypes.data, checksums[serial].ctypes.data,
                                     C.byref(err))
        assert not err.value, err.value
        ticks["serial pop" if serial else "subtree pop"] = pops
    for entries_per_lane in (4, 8, 16):
        ticks[entries_per_lane], accepted[entries_per_lane] = np.zeros(waves, dtype=np.uint64), np.zeros(waves, dtype=np.uint64)
        err = C.c_char_p()
        hooks.usearch_amd_bench_top(entries_per_lane, count, limit, waves, ticks[entries_per_lane].ctypes.data,
                                    accepted[entries_per_lane].ctypes.data, C.byref(err))
        assert not err.value, err.value
    return checksums, ticks, accepted


def test_micro_benchmark_hooks_report_every_wave():
    waves, count, limit = 3, 64, 16
    checksums, ticks, accepted = micro_benchmarks(waves, 32, count, limit)
    assert np.array_equal(checksums[0], checksums[1]) and checksums[0].all(), "the two pops disagree on what they popped"
    assert len(set(checksums[0].tolist())) == waves  # every wave draws its own keys
    assert all(t.all() for t in ticks.values())  # every wave wrote its clock
    for entries_per_lane in (4, 8, 16):  # the first `limit` candidates are always taken
        assert ((accepted[entries_per_lane] >= limit) & (accepted[entries_per_lane] <= count)).all()
