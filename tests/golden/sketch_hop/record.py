"""Writes counters.json next to itself: `stats.sketch_tested`, `stats.sketch_pruned` and Σ visited of every case of
tests/test_gpu_sketch_hop.py, as the library loaded counts them. Run once, on a GPU, from the repository root with the library of
the commit BEFORE the sketch hop changed (USEARCH_AMD_LIBRARY=<that build's libusearch_amd.so>):

    python tests/golden/sketch_hop/record.py

Every sameness check of a case runs on the way, so a recording is only written from a library that passes them."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(HERE))))

from tests import test_gpu_sketch_hop as cases  # noqa: E402

if __name__ == "__main__":
    recorded = {name: cases.run(name) for name in list(cases.CASES) + list(cases.SPECIAL)}
    for name, runs in recorded.items():
        for run_name, c in runs.items():
            print(f"{name} {run_name}: survivors per hop {(c['tested'] - c['pruned']) / max(1, c['visited']):.2f}")
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "counters.json")
    with open(out, "w") as file:
        json.dump(recorded, file, indent=1, sort_keys=True)
        file.write("\n")
    print(f"wrote {out}")
