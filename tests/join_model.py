"""A literal restatement of the reference's semantic join, `unum::usearch::join` (the reference's include/usearch/index.hpp:4359-4545),
one proposal at a time. It is the yardstick of the device's join (usearch_amd/csrc/join.hip), which reaches the same matching
through one search per man and parallel rounds.

The loop, line by line:
- the smaller collection proposes; on equal sizes `a` does; the result still maps `a` to `b` (4373-4385);
- `max_proposals == 0` becomes log(men) + threads, assigned to a size_t (4390-4391), then capped at the men's size (4394);
- a FIFO queue starts with every man (4406-4409); a man with c proposals so far searches the women with k = c + 1 and proposes to
  the last result, `candidates.back()` (4465-4480); a man who used up max_proposals stays single (4458-4460);
- a free woman accepts; an engaged woman recomputes her husband's distance with her own row first and switches only when it is
  strictly larger than the proposal's (4482-4510); the loser goes back into the queue.

`search(man, k)` → list of (woman, distance), nearest first, at most k long; `distance(woman, man)` → the recomputed distance.
Men and women are indices; `proposers` lists the men that take part (all by default — the device leaves tombstoned men out).
"""
from __future__ import annotations

import math
import random
from collections import deque
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

Search = Callable[[int, int], Sequence[Tuple[int, float]]]
Distance = Callable[[int, int], float]


def default_max_proposals(men: int, max_proposals: int = 0, threads: int = 1) -> int:
    """index.hpp:4390-4394: log(men) + executor.size() truncated to an integer, then at most `men`."""
    if max_proposals == 0 and men:
        max_proposals = int(math.log(men) + threads)
    return min(men, max_proposals)


def stable_marriage(men: int, search: Search, distance: Distance, max_proposals: int, order: str = "fifo",
                    seed: Optional[int] = None, proposers: Optional[Iterable[int]] = None) -> Dict[int, int]:
    """The proposal loop of index.hpp:4414-4521 for `men` men → {man: woman}. `order` picks which free man proposes next:
    "fifo" (the reference's ring), "reversed" (the ring started backwards) or "random" (a seeded random free man each time) —
    with strict preferences the outcome is the same whatever the order."""
    queue = list(range(men)) if proposers is None else list(proposers)
    if order == "reversed":
        queue.reverse()
    queue = deque(queue)
    rng = random.Random(seed)
    proposals = [0] * men
    man_to_woman: Dict[int, int] = {}
    woman_to_man: Dict[int, int] = {}
    while queue:
        if order == "random":
            j = rng.randrange(len(queue))
            queue[j], queue[-1] = queue[-1], queue[j]
            man = queue.pop()
        else:
            man = queue.popleft()
        if proposals[man] >= max_proposals:
            continue
        proposals[man] += 1
        candidates = search(man, proposals[man])
        if not candidates:
            continue
        woman, d = candidates[-1]
        husband = woman_to_man.get(woman)
        if husband is None:
            man_to_woman[man] = woman
            woman_to_man[woman] = man
        elif distance(woman, husband) > d:
            del man_to_woman[husband]
            man_to_woman[man] = woman
            woman_to_man[woman] = man
            queue.append(husband)
        else:
            queue.append(man)
    return man_to_woman


def join(size_a: int, size_b: int, search_b: Search, search_a: Search, distance_b_to_a: Distance, distance_a_to_b: Distance,
         max_proposals: int = 0, threads: int = 1, order: str = "fifo", seed: Optional[int] = None,
         proposers_a: Optional[Iterable[int]] = None, proposers_b: Optional[Iterable[int]] = None) -> Dict[int, int]:
    """`join(a, b)` → {a: b}. `search_b(a_member, k)` searches `b` with a member of `a`, `search_a` the other way;
    `distance_b_to_a(b_member, a_member)` is the metric with `b`'s row first (a woman of `b` recomputing her husband from `a`)."""
    if size_b < size_a:  # index.hpp:4373-4385: `b` proposes, the result is turned back into a → b
        p = default_max_proposals(size_b, max_proposals, threads)
        matched = stable_marriage(size_b, search_a, distance_a_to_b, p, order, seed, proposers_b)
        return {a: b for b, a in matched.items()}
    p = default_max_proposals(size_a, max_proposals, threads)
    return stable_marriage(size_a, search_b, distance_b_to_a, p, order, seed, proposers_a)


def weakly_stable(matching: Dict[int, int], lists: Dict[int, List[Tuple[int, float]]], distance: Distance) -> List[Tuple[int, int]]:
    """Blocking pairs of `matching` ({man: woman}) under the men's lists ({man: [(woman, d), …]}): a man who strictly prefers a
    listed woman who is free or who strictly prefers him to her husband (`distance(woman, man)` → her view). → the pairs found."""
    husband_of = {w: m for m, w in matching.items()}
    blocking = []
    for man, entries in lists.items():
        own = matching.get(man)
        own_d = next((d for w, d in entries if w == own), math.inf) if own is not None else math.inf
        for woman, d in entries:
            if not d < own_d:
                break
            husband = husband_of.get(woman)
            if husband is None or distance(woman, man) < distance(woman, husband):
                blocking.append((man, woman))
    return blocking


# The joins the GPU tests run (tests/test_gpu_join.py) and the CPU tests tie to the reference (tests/test_join_model.py):
# (metric, dtype, ndim, |a|, |b|, max_proposals, expansion, exact). Seeds: `a` = SEED_A, `b` = SEED_B; keys of `a` start at
# KEYS_A, of `b` at KEYS_B, so that a swapped pair cannot pass unnoticed.
CASES = [
    ("cos", "f32", 32, 400, 600, 0, 64, False),   # |a| < |b|, the default P
    ("l2sq", "f16", 48, 600, 400, 6, 64, False),  # |a| > |b|: the roles swap, the output still maps a → b
    ("ip", "bf16", 32, 500, 500, 5, 64, False),   # |a| = |b|: a proposes
    ("cos", "f32", 32, 500, 700, 12, 8, False),   # P > expansion: proposals 9 … 12 from searches of their own
    ("l2sq", "f16", 48, 400, 500, 8, 64, True),   # exact lists
    ("ip", "bf16", 32, 300, 250, 0, 64, True),    # exact, roles swapped, the default P
]
SEED_A, SEED_B = 31, 32
KEYS_A, KEYS_B = 1000, 100000


def lanes_per_row(dtype: str, ndim: int) -> int:
    """The kernels' lanes per stored row (engine.hip `row_geometry`): the oracle restates their summation layout with it."""
    bits = {"f32": 32, "f64": 64, "f16": 16, "bf16": 16, "i8": 8, "b1": 1}[dtype]
    chunks = max(1, (ndim * bits // 8 + 15) // 16)
    lanes = min(8, 1 << (chunks - 1).bit_length())
    return min(2, lanes) if chunks <= 8 else lanes
