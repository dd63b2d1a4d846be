"""The table update alone: the dense route against the row-sparse (lazy) Adam step, at the table of BASELINE configs[3]
(V 1 M, D 256) and of configs[1] (V 100 k, D 128), for the rows one step of configs[3] names: n = 1024 * 50 lookups + 15 000 head
rows, Zipf(1.0) over the table.

One process per shape (started by the driver under its own time limit), device events, the three legs alternated inside every
iteration so that a drift of the box hits all alike:

  dense   what FusedAdam's table bucket runs: ops.scatter_rows_sorted of (ids, rows) into the [V, D] gradient (sort + segmented
          sum) + ops.adam_step_ over the whole bucket, which also zeroes the gradient again.  At least 7 V D 4 bytes: param,
          exp_avg, exp_avg_sq read and written, the gradient read and zeroed.
  lazy    ops.row_adam_step_ on the same (ids, rows), sort included (csrc/row_adam.hip).  About (n + 8 U) D 4 bytes for U distinct
          rows -- n gradient rows read, the compact gradient written and read, three table rows read and written -- plus the sort.

  clipped the same step in its two halves with the global norm in between (include/t4r_hip_rowclip.h): ops.row_adam_reduce_ (sort,
          stages 1 and 2, the sum of squares of the compact rows) + ops.grad_clip_coef_ over its partials + ops.row_adam_apply_ with
          the device coefficient (max_norm = inf: the coefficient is 1 and the bits are the lazy leg's).  The model adds one read of
          the compact buffer, 4 U D bytes, and two launches (the sum of squares, the one-workgroup coefficient) to the lazy leg.

Before anything is timed the legs run once from one state and the rows that have a gradient are compared bit for bit.

    python tools/row_adam_bench.py [--iters 50] [--warmup 10] [--out profiles/row_adam_ab.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1_000_000, 256), (100_000, 128)]
N_LOOKUPS = 1024 * 50 + 15_000
N_ID_SETS = 4


def zipf_ids(V, n, g, dev):
    import torch

    w = 1.0 / torch.arange(1, V + 1, device=dev, dtype=torch.float64)
    cdf = torch.cumsum(w, 0) / w.sum()
    rank = torch.searchsorted(cdf, torch.rand(n, generator=g, device=dev, dtype=torch.float64)).clamp_(max=V - 1)
    return torch.randperm(V, generator=g, device=dev)[rank]        # popular items anywhere in the table


def one(V, D, iters, warmup):
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("row_adam_bench needs the GPU: a CPU run measures nothing")
    from transformers4rec_amd import ops

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    n = N_LOOKUPS
    sets = [(zipf_ids(V, n, g, dev), 1e-3 * torch.randn(n, D, generator=g, device=dev)) for _ in range(N_ID_SETS)]
    uniq = [int(torch.unique(i).numel()) for i, _ in sets]
    p0 = 0.05 * torch.randn(V, D, generator=g, device=dev)
    dense = dict(p=p0.clone(), g=torch.zeros(V, D, device=dev), m=torch.zeros(V, D, device=dev), v=torch.zeros(V, D, device=dev))
    lazy = dict(p=p0.clone(), m=torch.zeros(V, D, device=dev), v=torch.zeros(V, D, device=dev))
    clip = dict(p=p0.clone(), m=torch.zeros(V, D, device=dev), v=torch.zeros(V, D, device=dev))
    part = torch.zeros(ops.row_grad_sumsq_parts(n, D), device=dev, dtype=torch.float64)
    out2 = torch.zeros(2, device=dev)
    del p0
    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)

    def leg_dense(ids, rows, step):
        ops.scatter_rows_sorted(dense["g"], ids, rows)
        ops.adam_step_(dense["p"].view(-1), dense["g"].view(-1), dense["m"].view(-1), dense["v"].view(-1), step, zero_grad=True, **hp)

    def leg_lazy(ids, rows, step):
        ops.row_adam_step_(lazy["p"], lazy["m"], lazy["v"], ids, rows, step, **hp)

    def leg_clipped(ids, rows, step):
        cnt, st = ops.row_adam_reduce_(ids, rows, V, -1, part)
        ops.grad_clip_coef_(part, cnt, 1.0, float("inf"), out2)
        ops.row_adam_apply_(clip["p"], clip["m"], clip["v"], st, step, clip_coef=out2[1:], **hp)

    # same results first: one step from one state, the rows that have a gradient bit for bit (every other row has zero moments
    # and a zero gradient in the dense leg: it does not move there either)
    leg_dense(*sets[0], 1)
    leg_lazy(*sets[0], 1)
    leg_clipped(*sets[0], 1)
    torch.cuda.synchronize()
    same = all(bool(torch.equal(dense[k].view(torch.int32), other[k].view(torch.int32))) for k in ("p", "m", "v") for other in (lazy, clip))
    same = same and float(out2[1]) == 1.0
    if not same:
        raise SystemExit(f"row_adam_bench: the legs disagree after one step at V={V} D={D}; nothing timed")

    legs = {"dense": leg_dense, "lazy": leg_lazy, "clipped": leg_clipped}
    times = {k: [] for k in legs}
    order = list(legs)
    for it in range(warmup + iters):
        ids, rows = sets[it % N_ID_SETS]
        for name in order[it % 3:] + order[:it % 3]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            legs[name](ids, rows, it + 2)
            e1.record()
            e1.synchronize()
            if it >= warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)

    def stats(v):
        v = sorted(v)
        return {"median_us": round(statistics.median(v), 2), "p10_us": round(v[len(v) // 10], 2), "p90_us": round(v[len(v) * 9 // 10], 2)}

    res = {k: stats(v) for k, v in times.items()}
    U = sum(uniq) / len(uniq)
    return {"V": V, "D": D, "n": n, "distinct_rows_mean": round(U, 1), "first_step_bits_equal": same, "legs": res,
            "dense_over_lazy": round(res["dense"]["median_us"] / res["lazy"]["median_us"], 2),
            "outside_spread": res["lazy"]["p90_us"] < res["dense"]["p10_us"],
            "clipped_minus_lazy_us": round(res["clipped"]["median_us"] - res["lazy"]["median_us"], 2),
            "clipped_norm": round(float(out2[0]), 6),
            "model_bytes": {"dense_at_least": 7 * V * D * 4, "lazy_about": int((n + 8 * U) * D * 4) + 2 * n * 4,
                            "clipped_adds_about": int(U * D * 4)},
            "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "row_adam_ab.json"))
    ap.add_argument("--one", nargs=2, type=int, metavar=("V", "D"), help="time one shape in this process and print its record")
    ap.add_argument("--timeout", type=int, default=240, help="seconds each shape's process may take")
    args = ap.parse_args()
    if args.one:
        print(json.dumps(one(args.one[0], args.one[1], args.iters, args.warmup)))
        return
    shapes = []
    for V, D in SHAPES:
        # a fresh process per shape, under its own time limit; a shape that fails ends the run: nothing more starts on the GPU
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(V), str(D), "--iters", str(args.iters),
                            "--warmup", str(args.warmup)], capture_output=True, text=True, timeout=args.timeout)
        if r.returncode != 0:
            raise SystemExit(f"row_adam_bench: V={V} D={D} ended with {r.returncode}\n{r.stdout}\n{r.stderr}")
        shapes.append(json.loads(r.stdout.strip().splitlines()[-1]))
    record = {"tool": "tools/row_adam_bench.py", "iters": args.iters, "warmup": args.warmup,
              "timing": "device events around each leg, one process per shape, the three legs alternated within every iteration; microseconds",
              "ids": f"Zipf(1.0) over the table, {N_ID_SETS} sets of n = 1024 * 50 + 15 000 rotated over the iterations",
              "shapes": shapes}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
