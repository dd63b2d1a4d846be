#!/usr/bin/env python
"""What an item filter costs inside the collect pass: ops.item_topk with allow_bits / exclude (the filtered heads of
include/t4r_hip_filter.h) against the unfiltered ops.item_topk of the same process and against the materialised composition
(item_scores -> item_mask_ -> topk), at 1024 x 100 001 x 128 and 1024 x 1 000 001 x 256, k 20, fp32 table and fp16 serving image.
One process, the legs interleaved, device events, median (minimum) microseconds, rows that fell back per leg.

    python tools/item_filter_bench.py --out profiles/item_filter_ab.json
"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--shapes", default="100001x128,1000001x256", help="comma-separated VxD")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from transformers4rec_amd import ops  # noqa: E402

N, K, E = 1024, 20, 20


def time_legs(legs, reps):
    """({name: [us per repetition]}, {name: fallback rows of the leg's last call}): every repetition runs every leg once, in turn"""
    fallback = {}
    for name, fn in legs.items():
        fn()
        fallback[name] = ops.item_topk_stats()["fallback_rows"] if name != "composition_p0.5" else None
    torch.cuda.synchronize()
    out = {k: [] for k in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) * 1e3)
    return out, fallback


rows = []
g = torch.Generator(device="cuda").manual_seed(0)
for shape in args.shapes.split(","):
    V, D = (int(v) for v in shape.split("x"))
    x = torch.randn((N, D), device="cuda", generator=g)
    W32 = torch.randn((V, D), device="cuda", generator=g) * 0.1
    u = torch.rand(V, device="cuda", generator=g)
    bits = {"all": ops.pack_item_filter(torch.ones(V, dtype=torch.bool, device="cuda")),
            "p0.5": ops.pack_item_filter(u < 0.5), "p0.05": ops.pack_item_filter(u < 0.05)}
    for table in ("fp32", "fp16"):
        W = W32 if table == "fp32" else ops.pack_item_table(W32, "fp16")
        seen = ops.item_topk(x, W, E)[1]              # the lists that matter: each row's own best items
        legs = {"item_topk": lambda: ops.item_topk(x, W, K),
                "filtered_all_bits": lambda: ops.item_topk(x, W, K, allow_bits=bits["all"]),
                "filtered_p0.5": lambda: ops.item_topk(x, W, K, allow_bits=bits["p0.5"]),
                "filtered_p0.05": lambda: ops.item_topk(x, W, K, allow_bits=bits["p0.05"]),
                "filtered_lists_E20": lambda: ops.item_topk(x, W, K, exclude=seen)}

        def composition():
            with ops.precision("fp32"):
                s = ops.item_scores(x, W)             # a fresh buffer: masked in place, no copy
            return ops.topk(ops.item_mask_(s, bits["p0.5"], seen), K)
        legs["composition_p0.5"] = composition
        t, fb = time_legs(legs, args.reps)
        row = dict(N=N, V=V, D=D, k=K, table=table,
                   **{f"{n}_us_median": round(statistics.median(v), 1) for n, v in t.items()},
                   **{f"{n}_us_min": round(min(v), 1) for n, v in t.items()},
                   **{f"{n}_fallback_rows": r for n, r in fb.items() if r is not None})
        rows.append(row)
        print(json.dumps(row), flush=True)
        del W
    del W32, x
res = dict(tool="tools/item_filter_bench.py", reps=args.reps, device=torch.cuda.get_device_name(0), rows=rows)
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
