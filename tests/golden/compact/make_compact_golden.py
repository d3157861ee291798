"""One-off: records tests/golden/compact/*.npz with the driver of make_compact_golden.cpp (compile it as its header says).

    python tests/golden/compact/make_compact_golden.py <path of the compiled driver>

Every fixture holds two images of one small index the reference built on one thread (cos, f32 × 8, key = 1000 + row): `before`,
saved after the removals, and `after`, saved after the reference's own `isolate()`; plus the removed keys. Not run by any test.
(The fixtures have a folder of their own: tests/fuzz/ takes every .npz directly under tests/golden/ for an index image.)
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", ".."))
from oracle import oraclebind  # noqa: E402

NDIM = 8


def record(driver: str, scratch: str, n: int, connectivity: int, seed: int, removed: np.ndarray):
    X = np.random.default_rng(seed).standard_normal((n, NDIM)).astype(np.float32)
    X.tofile(os.path.join(scratch, "X.bin"))
    np.asarray(removed, dtype=np.uint64).tofile(os.path.join(scratch, "removed.bin"))
    before, after = os.path.join(scratch, "before.usearch"), os.path.join(scratch, "after.usearch")
    subprocess.check_call([driver, os.path.join(scratch, "X.bin"), str(n), str(NDIM), str(connectivity),
                           os.path.join(scratch, "removed.bin"), str(len(removed)), before, after])
    return np.fromfile(before, dtype=np.uint8), np.fromfile(after, dtype=np.uint8)


def main(driver: str) -> None:
    with tempfile.TemporaryDirectory() as scratch:
        cases = {}
        # alternate keys removed: the reference's own `test_isolate` (cpp/test.cpp:1147-1180), larger
        cases["alternate_keys"] = (300, 8, 51, 1000 + np.arange(0, 300, 2))
        # the entry point among the removed: found in an image saved with nothing removed
        whole, _ = record(driver, scratch, 400, 4, 52, [])
        index = oraclebind.OracleIndex(whole)
        entry_key = index.key(int(index.ix.entry_slot))
        others = 1000 + np.random.default_rng(53).choice(400, 60, replace=False)
        cases["entry_point_removed"] = (400, 4, 52, np.unique(np.append(others, entry_key)))
        cases["one_removed"] = (250, 6, 54, np.array([1000 + 17]))
        for name, (n, connectivity, seed, removed) in cases.items():
            before, after = record(driver, scratch, n, connectivity, seed, removed)
            np.savez_compressed(os.path.join(HERE, name + ".npz"), before=before, after=after, removed=np.asarray(removed, dtype=np.uint64))
            print(name, len(before), os.path.getsize(os.path.join(HERE, name + ".npz")))


if __name__ == "__main__":
    main(sys.argv[1])
