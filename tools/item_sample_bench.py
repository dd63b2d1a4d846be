#!/usr/bin/env python
"""What the Gumbel noise costs inside the collect pass: ops.item_sample (fused sampling head) against its materialised
composition (item_scores -> gumbel_add_ -> topk) and against ops.item_topk, at N 1024, D 128, V 100 001 / 1 000 001, k 1 / 20,
fp32 table and fp16 serving image.  One process, the legs interleaved, device events, median (minimum) microseconds.

    python tools/item_sample_bench.py --out profiles/item_sample_ab.json
    python tools/item_sample_bench.py --tree /path/to/parent/checkout --only-topk      # item_topk of another (built) checkout
"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--tree", help="time this (built) checkout's package instead of the tool's own")
ap.add_argument("--only-topk", action="store_true", help="time ops.item_topk alone (a checkout without the sampling heads)")
args = ap.parse_args()
sys.path.insert(0, args.tree or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from transformers4rec_amd import ops  # noqa: E402

N, D = 1024, 128
SEED, CTR = 1234, (1 << 16) | (255 << 8) | 7


def time_legs(legs, reps):
    """{name: [us per repetition]}: every repetition runs every leg once, in turn"""
    for fn in legs.values():
        fn()
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
    return out


rows = []
g = torch.Generator(device="cuda").manual_seed(0)
x = torch.randn((N, D), device="cuda", generator=g)
for V in (100001, 1000001):
    W32 = torch.randn((V, D), device="cuda", generator=g) * 0.1
    for table in ("fp32", "fp16"):
        W = W32 if table == "fp32" else ops.pack_item_table(W32, "fp16")
        for k in (1, 20):
            legs = {"item_topk": lambda: ops.item_topk(x, W, k)}
            if not args.only_topk:
                legs["item_sample"] = lambda: ops.item_sample(x, W, k, SEED, CTR)

                def composition():
                    # (item_scores returns a fresh buffer: the noise goes into it in place, no copy)
                    with ops.precision("fp32"):
                        s = ops.item_scores(x, W)
                    return ops.topk(ops.gumbel_add_(s, SEED, CTR), k)
                legs["composition"] = composition
            t = time_legs(legs, args.reps)
            row = dict(N=N, V=V, D=D, k=k, table=table,
                       **{f"{n}_us_median": round(statistics.median(v), 1) for n, v in t.items()},
                       **{f"{n}_us_min": round(min(v), 1) for n, v in t.items()})
            if not args.only_topk:
                row["fallback_rows"] = ops.item_topk_stats()["fallback_rows"]
            rows.append(row)
            print(json.dumps(row), flush=True)
        del W
    del W32
res = dict(tool="tools/item_sample_bench.py", tree=args.tree or "this", reps=args.reps, device=torch.cuda.get_device_name(0), rows=rows)
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
