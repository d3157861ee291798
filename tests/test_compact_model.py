"""The plain model of `isolate` / `compact` (tests/compact_model.py) pinned down without a GPU: `isolate` against what the
compiled reference did (fixtures under tests/golden/compact/, recorded by make_compact_golden.{cpp,py} there), `compact` by the
invariants compact.hpp states."""
import os

import numpy as np
import pytest

from tests import compact_model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compact")
FIXTURES = ["alternate_keys", "entry_point_removed", "one_removed"]
FREE, NONE = compact_model.FREE_KEY, compact_model.NONE_SLOT


def load(name):
    fixture = np.load(os.path.join(GOLDEN, name + ".npz"))
    return fixture["before"], fixture["after"], fixture["removed"]


@pytest.mark.parametrize("name", FIXTURES)
def test_isolate_is_the_references_list_for_list(name):
    before, after, removed = load(name)
    lists, levels, keys, entry, max_level = compact_model.read_image(before)
    assert sorted(1000 + slot for slot, key in enumerate(keys) if key == FREE) == sorted(removed.tolist())
    if name == "entry_point_removed":
        assert keys[entry] == FREE
    expected_lists, expected_levels, expected_keys, expected_entry, expected_max_level = compact_model.read_image(after)
    got, erased = compact_model.isolate(lists, keys)
    assert erased > 0
    for slot in range(len(keys)):  # every slot, removed members' own lists included, every level
        assert got[slot] == expected_lists[slot], f"slot {slot}: the model says {got[slot]}, the reference wrote {expected_lists[slot]}"
    assert erased == sum(len(a) - len(b) for old, new in zip(lists, expected_lists) for a, b in zip(old, new))
    # nothing else moved
    assert (expected_levels, expected_keys, expected_entry, expected_max_level) == (levels, keys, entry, max_level)


@pytest.mark.parametrize("name", FIXTURES)
def test_compact_keeps_its_rules(name):
    before, _, _ = load(name)
    lists, levels, keys, entry, max_level = compact_model.read_image(before)
    isolated, erased = compact_model.isolate(lists, keys)
    out = compact_model.compact(lists, levels, keys, entry)
    survivors = [slot for slot, key in enumerate(keys) if key != FREE]
    # the slot map is the rank among the survivors
    assert [out["slot_map"][slot] for slot in survivors] == list(range(len(survivors)))
    assert all(out["slot_map"][slot] == NONE for slot, key in enumerate(keys) if key == FREE)
    assert out["keys"] == [keys[slot] for slot in survivors] and out["levels"] == [levels[slot] for slot in survivors]
    assert (out["pruned_edges"], out["removed_members"]) == (erased, len(keys) - len(survivors))
    # every new list is the isolated list, mapped; no cell names a removed member
    for new_slot, old_slot in enumerate(survivors):
        assert len(out["lists"][new_slot]) == levels[old_slot] + 1
        for level, cells in enumerate(out["lists"][new_slot]):
            assert cells == [out["slot_map"][cell] for cell in isolated[old_slot][level]]
            assert all(cell < len(survivors) for cell in cells)
            assert all(out["levels"][cell] >= level for cell in cells)
    # the entry rule
    if keys[entry] != FREE:
        assert (out["entry"], out["max_level"]) == (out["slot_map"][entry], max_level)
    else:
        top = max(out["levels"])
        assert (out["entry"], out["max_level"]) == (out["levels"].index(top), top)


def test_compact_of_nothing_and_of_everything():
    lists = [[[1, 2]], [[0, 2], [2]], [[1, 0], [1]]]
    levels, keys = [0, 1, 1], [10, 11, 12]
    same = compact_model.compact(lists, levels, keys, 1)
    assert same["lists"] == lists and same["slot_map"] == [0, 1, 2] and (same["entry"], same["max_level"]) == (1, 1)
    assert same["pruned_edges"] == 0 and same["removed_members"] == 0
    gone = compact_model.compact(lists, levels, [FREE] * 3, 1)
    assert gone["lists"] == [] and gone["slot_map"] == [NONE] * 3 and (gone["entry"], gone["max_level"]) == (0, 0)
    assert gone["pruned_edges"] == 8 and gone["removed_members"] == 3
    # the entry point leaves: the lowest slot of the highest level among the survivors; order inside a list is kept
    one = compact_model.compact(lists, levels, [10, FREE, 12], 1)
    assert one["lists"] == [[[1]], [[0], []]] and one["slot_map"] == [0, NONE, 1] and (one["entry"], one["max_level"]) == (1, 1)
