#!/usr/bin/env python
"""One-pass evaluation head over the serving image, A / B in one process (in the manner of tools/infer_topk_bench.py).

    python tools/item_eval_bench.py [--reps 30] [--out profiles/item_eval_h16_ab.json] [--shapes small,mid,large]
    python tools/item_eval_bench.py --trace-shape mid --reps 10      # the workload of a kernel-trace run (no timing)

Legs, interleaved after a warm-up of each, every repetition timed with device events; minimum and median per leg:
  E     ops.item_eval(x, image, labels): lse, target, score sum and rank in one pass over the 16-bit image
  F32   the fused fp32 pieces for the same result: ops.rank_of_target + ops.linear_softmax_ce_fwd (two passes over the fp32 table)
  A16   ops.item_scores(x, image) + torch.logsumexp + the rank comparison over the materialised [N, V] scores (where they fit)
  T     ops.item_topk(x, image, 10): the bare pass over the same image (informational)
fp16 at every shape, bf16 at `--bf16-shape` (default mid).  Also recorded: the largest |lse - logsumexp64(item_scores)| over the
first 64 rows, exact equality of target / rank there, and the workspace against the [N, V] score matrix."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from transformers4rec_amd import ops  # noqa: E402

SHAPES = {"small": (1024, 100001, 128), "mid": (1024, 1000001, 256), "large": (256, 10000001, 512)}


def make(N, V, D):
    g = torch.Generator(device="cuda").manual_seed(N + V + D)
    x = torch.randn((N, D), device="cuda", generator=g)
    W = torch.empty((V, D), device="cuda")
    step = 1 << 20                        # in slabs: torch.randn's own scratch stays small next to a 20 GB table
    for s in range(0, V, step):
        W[s: s + step] = torch.randn((min(step, V - s), D), device="cuda", generator=g) * 0.1
    y = torch.randint(0, V, (N,), device="cuda", generator=g)
    return x, W, y


def fits(nbytes):
    free, _ = torch.cuda.mem_get_info()
    return nbytes < 0.9 * free


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3      # us


def a16(x, im, y):
    S = ops.item_scores(x, im)
    lse = torch.logsumexp(S, dim=1)
    t = torch.gather(S, 1, y[:, None])
    cols = torch.arange(S.shape[1], device=S.device)[None, :]
    rank = ((S > t) | ((S == t) & (cols < y[:, None]))).sum(dim=1)
    return lse, t[:, 0], S.sum(dim=1), rank


def check(x, im, y, rows=64):
    """E against the materialised scores on the first rows: (target bits equal, ranks equal, largest lse error, largest
    score_sum error over its 2e-5 * sum |S| bound)"""
    lse, target, ssum, rank = ops.item_eval(x, im, y)
    S = ops.item_scores(x[:rows], im)
    yy = y[:rows]
    t = torch.gather(S, 1, yy[:, None])[:, 0]
    cols = torch.arange(S.shape[1], device=S.device)[None, :]
    r = ((S > t[:, None]) | ((S == t[:, None]) & (cols < yy[:, None]))).sum(dim=1)
    e_lse, e_sum = 0.0, 0.0
    for r0 in range(0, rows, 16):                                # fp64 in row blocks (memory)
        Sd = S[r0:r0 + 16].double()
        e_lse = max(e_lse, float((lse[r0:r0 + 16].double() - torch.logsumexp(Sd, dim=1)).abs().max()))
        e_sum = max(e_sum, float(((ssum[r0:r0 + 16].double() - Sd.sum(dim=1)).abs() / (2e-5 * Sd.abs().sum(dim=1))).max()))
    return (bool(torch.equal(target[:rows].view(torch.int32), t.view(torch.int32))), bool(torch.equal(rank[:rows].long(), r)),
            e_lse, e_sum)


def bench_shape(name, dtypes, reps):
    N, V, D = SHAPES[name]
    rec = dict(shape=name, N=N, V=V, D=D, reps=reps)
    if not fits(4 * V * D + 2 * V * ops.image_ld(D) + (1 << 30)):
        rec["skipped"] = "the item table and its image do not fit the device"
        return rec
    x, W, y = make(N, V, D)
    scores_bytes = 4 * N * ops.pad_ld(V)
    legs = {"F32": lambda: (ops.rank_of_target(x, W, y), ops.linear_softmax_ce_fwd(x, W, y, 1.0, 0.0))}
    images = {dt: ops.pack_item_table(W, dt) for dt in dtypes}
    for dt, im in images.items():
        legs[f"E_{dt}"] = (lambda im: (lambda: ops.item_eval(x, im, y)))(im)
        legs[f"T_{dt}"] = (lambda im: (lambda: ops.item_topk(x, im, 10)))(im)
        if fits(3 * scores_bytes):
            legs[f"A16_{dt}"] = (lambda im: (lambda: a16(x, im, y)))(im)
        else:
            rec["A16_skipped"] = f"the {scores_bytes / 1e9:.1f} GB score matrix and its temporaries do not fit next to the table"
    for fn in legs.values():              # warm-up: code objects, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for dt, im in images.items():
        eq_t, eq_r, e_lse, e_sum = check(x, im, y)
        rec[f"E_{dt}_check_first_64_rows"] = dict(target_bits_equal=eq_t, ranks_equal=eq_r, max_abs_lse_error=e_lse,
                                                  max_score_sum_error_over_bound=e_sum)
    t = {n: [] for n in legs}
    for _ in range(reps):
        for n, fn in legs.items():
            t[n].append(once(fn))
    for n, v in t.items():
        rec[n] = dict(min_us=round(min(v), 1), median_us=round(statistics.median(v), 1), max_us=round(max(v), 1))
    rec["workspace_mb"] = round(ops._lib.load().t4r_item_eval_h16_ws_bytes(N, V, D) / 1e6, 1)
    rec["scores_mb"] = round(scores_bytes / 1e6, 1)
    for dt in images:
        e = rec[f"E_{dt}"]
        for other in ("F32", f"A16_{dt}"):
            if other in rec:
                o = rec[other]
                spread = max(o["median_us"] - o["min_us"], e["median_us"] - e["min_us"])
                rec[f"E_{dt}_below_{other}_by_more_than_the_larger_spread"] = bool(o["median_us"] - e["median_us"] > spread)
                rec[f"{other}_over_E_{dt}"] = round(o["median_us"] / e["median_us"], 2)
        rec[f"E_over_T_{dt}"] = round(e["median_us"] / rec[f"T_{dt}"]["median_us"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--shapes", default="small,mid,large")
    ap.add_argument("--bf16-shape", default="mid")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-shape", default=None, help="run only E (fp16) of this shape a few times (profiler workload)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("item_eval_bench: no GPU visible; there is nothing to measure without one")
    if a.trace_shape:
        N, V, D = SHAPES[a.trace_shape]
        x, W, y = make(N, V, D)
        im = ops.pack_item_table(W, "fp16")
        del W
        for _ in range(a.reps):
            ops.item_eval(x, im, y)
        torch.cuda.synchronize()
        return
    out = []
    for name in a.shapes.split(","):
        rec = bench_shape(name, ["fp16", "bf16"] if name == a.bf16_shape else ["fp16"], a.reps)
        print(json.dumps(rec), flush=True)
        out.append(rec)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), results=out), f, indent=1)


if __name__ == "__main__":
    main()
