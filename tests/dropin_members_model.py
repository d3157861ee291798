"""A plain restatement of what the drop-in C ABI keeps on the host about its members (usearch_amd/csrc/members.hpp, driven by
usearch_amd/csrc/dropin.hip): a list of slots, each with a key and a row; the ring of slots a removal freed, oldest first; `multi`;
and the capacity. It mirrors the reference's `index_dense_gt` bookkeeping (index_dense.hpp:507 `free_keys_`, 1479-1511 remove,
2162-2200 `reindex_keys_`) and predicts, call for call, what `usearch_add / remove / rename / get / contains / count / size /
capacity / clear / load_buffer / view_buffer` return and which error string they give (tests/test_dropin_members.py).

The rules:
- a slot whose key is `FREE` is a tombstone: it counts for `capacity`, not for `size`, and no key names it;
- `add` checks, in this order: the free key, room, a duplicate (unless `multi`). There is room while there are fewer slots than the
  capacity OR the ring is not empty: the oldest freed slot is taken before a new one, and nothing grows on its own;
- an image's tombstones are in the ring from the moment it is opened, lowest slot first;
- `remove` frees every slot of the key; `rename` rewrites every slot of `source`, and is refused onto a key in use unless `multi`;
- `get` gives the rows of a key in slot order;
- `clear` and opening an image drop every member and the ring; the capacity never shrinks.

What is not specified. The slots one `remove` of a multi-key frees enter the ring in the order the key table names them, which no rule
fixes (the reference iterates a hash table there too). The model keeps such slots as one group; adds that retake them must all carry
the same key and row, so that the outcome is the same whichever slot each one lands in; anything else raises `Unspecified` instead of
guessing. `staged` says whether keys and rows have left the image (the library serializes an unstaged index from its image bytes).

Rows are kept as the caller hands them in (the stored form: the caller owns the casts). Written for clarity, not speed.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

FREE = 0xFFFFFFFFFFFFFFFF

OUT_OF_ROOM = "Reserve capacity ahead of insertions!"
DUPLICATE = "Duplicate keys not allowed in high-level wrappers"
FREE_KEY = "Free key is reserved"
IN_USE = "Renaming impossible, the key is already in use"


class Unspecified(Exception):
    """The script would observe the order in which one multi-key removal freed its slots."""


class Members:
    def __init__(self, multi: bool = False, capacity: int = 0):
        self.multi = multi
        self.capacity = capacity            # what `reserve` and opened images asked for; `usearch_capacity` adds the slots in use
        self.slots: List[list] = []         # [key, row] per slot
        self.ring: List[List[int]] = []     # groups of freed slots, oldest first; a group of several is one multi-key removal
        self.filling: Optional[Tuple[int, bytes]] = None  # (key, row) going into the partly retaken group at the head of the ring
        self.has_image = False
        self.staged = False

    # ---- what the entry points report
    def size(self) -> int:
        return sum(key != FREE for key, _ in self.slots)

    def reported_capacity(self) -> int:
        return max(self.capacity, len(self.slots))

    def slots_of(self, key: int) -> List[int]:
        return [] if key == FREE else [slot for slot, (k, _) in enumerate(self.slots) if k == key]

    def count(self, key: int) -> int:
        return len(self.slots_of(key))

    def contains(self, key: int) -> bool:
        return self.count(key) != 0

    def get(self, key: int, count: int) -> list:
        return [self.slots[slot][1] for slot in self.slots_of(key)[:count]]

    # ---- what changes the members
    def reserve(self, capacity: int) -> None:
        self.capacity = max(self.capacity, capacity)

    def open_image(self, keys: Sequence[int], rows: Sequence[bytes], multi: bool) -> None:
        """`load_buffer` / `view_buffer` of a valid image: its slots, tombstones included, replace everything."""
        self.slots = [[int(key), row] for key, row in zip(keys, rows)]
        self.ring = [[slot] for slot, (key, _) in enumerate(self.slots) if key == FREE]
        self.filling = None
        self.multi = multi
        self.capacity = max(self.capacity, len(self.slots))
        self.has_image, self.staged = True, False

    def clear(self) -> None:
        self.slots, self.ring, self.filling = [], [], None
        self.has_image, self.staged = False, False

    def _stage(self) -> None:
        self.staged, self.has_image = True, False

    def _settled(self) -> None:
        if self.filling is not None:
            raise Unspecified("a multi-key removal's slots are only partly retaken")

    def add(self, key: int, row: bytes) -> Optional[str]:
        """→ the error string, or None."""
        if key == FREE:
            return FREE_KEY
        at_capacity = len(self.slots) >= self.capacity
        if at_capacity and self.has_image and self.ring:
            self._stage()  # the image's tombstones are listed the moment they are needed as room
        if at_capacity and not self.ring:
            return OUT_OF_ROOM
        if not self.multi and self.contains(key):
            return DUPLICATE
        self._stage()
        if not self.ring:
            self.slots.append([key, row])
            return None
        group = self.ring[0]
        if len(group) > 1 or self.filling is not None:
            if self.filling is None:
                self.filling = (key, row)
            elif self.filling != (key, row):
                raise Unspecified("different members into the slots of one multi-key removal")
        self.slots[group.pop(0)] = [key, row]
        if not group:
            self.ring.pop(0)
            self.filling = None
        return None

    def remove(self, key: int) -> int:
        slots = self.slots_of(key)
        if not slots:
            return 0
        self._settled()
        self._stage()
        for slot in slots:
            self.slots[slot][0] = FREE
        self.ring.append(slots)
        return len(slots)

    def rename(self, source: int, target: int) -> Tuple[int, Optional[str]]:
        """→ (members renamed, the error string or None)."""
        if target == FREE:
            return 0, FREE_KEY
        slots = self.slots_of(source)
        if not slots:
            return 0, None
        if not self.multi and self.contains(target):
            return 0, IN_USE
        self._settled()
        self._stage()
        for slot in slots:
            self.slots[slot][0] = target
        return len(slots), None
