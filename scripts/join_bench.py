"""Semantic join at scale, the way the reference's cpp/bench.cpp:412-445 measures it: an index joined with a second snapshot of
the same image. Prints one JSON line: sizes, P and expansion, the seconds of the preference lists and of the matching, rounds
and proposals per man, `recall_join` (the share of keys matched to themselves) and the share left unmatched.

    python scripts/join_bench.py --n 1000000 --dim 768 --dtype f16 --metric cos
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--n", type=int, default=1_000_000)
    parser.add_argument("--dim", type=int, default=768)
    parser.add_argument("--dtype", default="f16")
    parser.add_argument("--metric", default="cos")
    parser.add_argument("--expansion", type=int, default=64)
    parser.add_argument("--max-proposals", type=int, default=0)
    parser.add_argument("--threads", type=int, default=0, help="the executor.size() term of the default P (0 counts as 1)")
    parser.add_argument("--exact", action="store_true")
    parser.add_argument("--connectivity", type=int, default=16)
    parser.add_argument("--expansion-add", type=int, default=128)
    parser.add_argument("--repeat", type=int, default=1, help="joins timed; the last one is reported")
    args = parser.parse_args()

    import torch

    import usearch_amd
    from bench import synthetic_vectors_device  # the headline's own data distribution

    device = torch.device("cuda:0")
    started = time.perf_counter()
    data = synthetic_vectors_device(args.n, args.dim, args.dtype, 42, device)
    keys = np.arange(args.n, dtype=np.uint64)
    built = usearch_amd.build(None, args.metric, args.dtype, keys=keys, connectivity=args.connectivity,
                              expansion_add=args.expansion_add, device=0, device_pointer=data.data_ptr(), count=args.n,
                              stride=data.stride(0), ndim=args.dim)
    del data
    torch.cuda.empty_cache()
    build_seconds = time.perf_counter() - started
    men = built.index
    women = usearch_amd.Index.restore(built.save_buffer())  # bench.cpp:421: `index.copy()`
    for _ in range(args.repeat):
        begin = time.perf_counter()
        a_keys, b_keys, stats = men.join_arrays(women, args.max_proposals, args.exact, expansion=args.expansion, threads=args.threads)
        seconds = time.perf_counter() - begin
    line = {
        "what": "join", "n": args.n, "dims": args.dim, "dtype": args.dtype, "metric": args.metric, "exact": args.exact,
        "P": int(stats.max_proposals), "expansion": int(stats.expansion), "list_width": int(stats.list_width),
        "seconds_total": round(seconds, 4), "seconds_lists": round(stats.seconds_lists, 4),
        "seconds_matching": round(stats.seconds_matching, 4),
        "matching_share": round(stats.seconds_matching / max(1e-9, stats.seconds_lists), 4),
        "rounds": int(stats.rounds), "proposals_per_man": round(stats.proposals / args.n, 4),
        "engagements": int(stats.engagements), "lazy_searches": int(stats.lazy_searches),
        "visited_per_man": round(stats.visited_members / args.n, 2), "computed_per_man": round(stats.computed_distances / args.n, 2),
        "pairs": int(stats.pairs), "recall_join": round(float(np.sum(a_keys == b_keys)) / args.n, 6),
        "unmatched": round(1.0 - len(a_keys) / args.n, 6), "frontier": int(stats.frontier), "build_seconds": round(build_seconds, 2),
    }
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
