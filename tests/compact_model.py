"""A plain model of `isolate` and `compact` (usearch_amd/csrc/compact.hpp), one cell at a time, on Python lists.

An index is `lists[slot][level]` = the neighbour slots of `slot` on `level` in order, `keys[slot]`, `levels[slot]` and the entry
point. The model is pinned to the compiled reference by tests/test_compact_model.py (isolate: list for list against fixtures the
reference recorded) and the device code is pinned to the model by tests/test_gpu_compact.py.
"""
from __future__ import annotations

FREE_KEY = 0xFFFFFFFFFFFFFFFF  # index_dense.hpp:513
NONE_SLOT = 0xFFFFFFFF


def isolate(lists, keys):
    """`index_dense_gt::isolate` (index_dense.hpp:1709-1720 → index.hpp:3700-3728): in every list of every member, removed ones
    included, every neighbour whose key is FREE_KEY is erased and the rest keeps its order (`erase_if`, index.hpp:2181-2194).
    → (new lists, number of cells erased)."""
    out, erased = [], 0
    for per_level in lists:
        kept_levels = []
        for cells in per_level:
            kept = []
            for cell in cells:
                if keys[cell] == FREE_KEY:
                    erased += 1
                else:
                    kept.append(cell)
            kept_levels.append(kept)
        out.append(kept_levels)
    return out, erased


def compact(lists, levels, keys, entry):
    """compact.hpp's rules. → dict(lists, keys, levels, entry, max_level, slot_map, pruned_edges, removed_members)."""
    isolated, erased = isolate(lists, keys)
    slot_map, survivors = [], 0
    for key in keys:
        if key == FREE_KEY:
            slot_map.append(NONE_SLOT)
        else:
            slot_map.append(survivors)
            survivors += 1
    new_lists, new_keys, new_levels = [], [], []
    for slot, key in enumerate(keys):
        if key == FREE_KEY:
            continue
        new_lists.append([[slot_map[cell] for cell in cells] for cells in isolated[slot]])
        new_keys.append(key)
        new_levels.append(levels[slot])
    if not survivors:
        new_entry, max_level = 0, 0
    elif slot_map[entry] != NONE_SLOT:
        new_entry, max_level = slot_map[entry], levels[entry]
    else:
        new_entry = 0
        for slot in range(survivors):  # the highest level, the lowest slot among equals
            if new_levels[slot] > new_levels[new_entry]:
                new_entry = slot
        max_level = new_levels[new_entry]
    return dict(lists=new_lists, keys=new_keys, levels=new_levels, entry=new_entry, max_level=max_level, slot_map=slot_map,
                pruned_edges=erased, removed_members=len(keys) - survivors)


def read_image(image):
    """An image (np.uint8) → (lists, levels, keys, entry, max_level) through the oracle's parser."""
    from oracle import oraclebind
    index = oraclebind.OracleIndex(image)
    n = len(index)
    levels = [index.level(slot) for slot in range(n)]
    keys = [index.key(slot) for slot in range(n)]
    lists = [[[int(cell) for cell in index.neighbors(slot, level)] for level in range(levels[slot] + 1)] for slot in range(n)]
    return lists, levels, keys, int(index.ix.entry_slot), int(index.ix.max_level)
