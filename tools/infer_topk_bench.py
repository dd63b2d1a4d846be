#!/usr/bin/env python
"""Inference top-k head, A / B in one process: the materialised path (ops.gemm into the padded [N, V] scores + ops.topk, at
the default precision mode and at form 0) against the fused head (ops.item_topk, no [N, V] tensor) over the fp32 table (B) and
over a half-precision serving image of it (H_fp16, H_bf16: ops.pack_item_table once, its time reported separately).

    python tools/infer_topk_bench.py [--reps 30] [--out profiles/item_topk_ab.json] [--shapes small,mid,large] [--ks 10,20,100]
    python tools/infer_topk_bench.py --trace-shape mid --k 20 --reps 5      # the workload of a kernel-trace run (no timing)
    python tools/infer_topk_bench.py --trace-shape mid --trace-h16 fp16     # ... of the 16-bit head alone (counter passes)

After a warm-up of every leg the legs are interleaved (A default, A form 0, B, A default, ...), each repetition timed with
device events; minimum and median per leg are reported.  Legs whose buffers do not fit the device are recorded as skipped
with the reason.  The candidate statistics (sample size M, list capacity, mean / max candidates per row, overflow rows) come
from one extra fused call with the per-row counts copied back."""
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
    return x, W


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


def bench_shape(name, k, reps):
    N, V, D = SHAPES[name]
    rec = dict(shape=name, N=N, V=V, D=D, k=k, reps=reps)
    if not fits(4 * V * D + (1 << 30)):
        rec["skipped"] = "the item table does not fit the device"
        return rec
    x, W = make(N, V, D)
    scores_bytes = 4 * N * ops.pad_ld(V)

    def a_default():
        return ops.topk(ops.gemm(x, W, False, True, ldc=ops.pad_ld(V)), k, V)

    def a_fp32():
        with ops.precision("fp32"):
            return ops.topk(ops.gemm(x, W, False, True, ldc=ops.pad_ld(V)), k, V)

    def b_fused():
        return ops.item_topk(x, W, k)

    legs = {"B_fused": b_fused}
    if fits(scores_bytes + (1 << 28)):
        legs = {"A_default": a_default, "A_fp32": a_fp32, "B_fused": b_fused}
    else:
        rec["A_skipped"] = f"the {scores_bytes / 1e9:.1f} GB score matrix does not fit next to the table"
    images = {}
    for dt in ("fp16", "bf16"):           # the serving images: packed once, outside the timed legs
        if not fits(2 * V * ops.image_ld(D) + (1 << 28)):
            rec[f"H_{dt}_skipped"] = "the image does not fit next to the table"
            continue
        ops.pack_item_table(W, dt)        # warm-up
        packs = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            images[dt] = ops.pack_item_table(W, dt)      # includes its finiteness check (one pass over the image)
            e1.record()
            torch.cuda.synchronize()
            packs.append(e0.elapsed_time(e1) * 1e3)
        rec[f"pack_{dt}_us"] = round(min(packs), 1)
        legs[f"H_{dt}"] = (lambda im: (lambda: ops.item_topk(x, im, k)))(images[dt])
    for fn in legs.values():              # warm-up: code objects, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    if "A_fp32" in legs:
        (bv, bi), (av, ai) = b_fused(), a_fp32()
        rec["B_equals_A_fp32"] = bool(torch.equal(bv, av) and torch.equal(bi, ai))
        del bv, bi, av, ai
    for dt, im in images.items():
        (hv, hi), (mv, mi) = ops.item_topk(x, im, k), ops.topk(ops.item_scores(x[:64], im), k)
        rec[f"H_{dt}_equals_materialised_first_64_rows"] = bool(torch.equal(hv[:64], mv) and torch.equal(hi[:64], mi))
        del hv, hi, mv, mi
    t = {n: [] for n in legs}
    for _ in range(reps):
        for n, fn in legs.items():
            t[n].append(once(fn))
    for n, v in t.items():
        rec[n] = dict(min_us=round(min(v), 1), median_us=round(statistics.median(v), 1), max_us=round(max(v), 1))
    ops.item_topk_collect_counts(True)
    b_fused()
    ops.item_topk_collect_counts(False)
    st = ops.item_topk_stats()
    rec["fused"] = dict(sample_rows=st["sample_rows"], list_capacity=st["list_capacity"], fallback_rows=st["fallback_rows"],
                        cand_mean=round(st["cand_sum"] / N, 1), cand_max=st["cand_max"],
                        workspace_mb=round(ops._lib.load().t4r_item_topk_ws_bytes(N, V, D, k) / 1e6, 1),
                        scores_mb=round(scores_bytes / 1e6, 1))
    for dt, im in images.items():
        ops.item_topk_collect_counts(True)
        ops.item_topk(x, im, k)
        ops.item_topk_collect_counts(False)
        st = ops.item_topk_stats()
        rec[f"fused_{dt}"] = dict(sample_rows=st["sample_rows"], list_capacity=st["list_capacity"],
                                  fallback_rows=st["fallback_rows"], cand_mean=round(st["cand_sum"] / N, 1), cand_max=st["cand_max"],
                                  workspace_mb=round(ops._lib.load().t4r_item_topk_h16_ws_bytes(N, V, D, k) / 1e6, 1),
                                  image_mb=round(2 * V * ops.image_ld(D) / 1e6, 1))
        b, h = rec["B_fused"], rec[f"H_{dt}"]
        spread = max(b["median_us"] - b["min_us"], h["median_us"] - h["min_us"])
        rec[f"H_{dt}_below_B_by_more_than_the_larger_spread"] = bool(b["median_us"] - h["median_us"] > spread)
        rec[f"B_over_H_{dt}"] = round(b["median_us"] / h["median_us"], 2)
    if "A_default" in rec:
        spread = rec["A_default"]["median_us"] - rec["A_default"]["min_us"]
        rec["B_below_A_default_by_more_than_A_spread"] = bool(rec["A_default"]["median_us"] - rec["B_fused"]["median_us"] > spread)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--shapes", default="small,mid,large")
    ap.add_argument("--ks", default="10,20,100")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-shape", default=None, help="run only the three legs of this shape a few times (profiler workload)")
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--trace-h16", default=None, help="with --trace-shape: run only the 16-bit head over a fp16 | bf16 image")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("infer_topk_bench: no GPU visible; there is nothing to measure without one")
    if a.trace_shape:
        N, V, D = SHAPES[a.trace_shape]
        x, W = make(N, V, D)
        if a.trace_h16:
            im = ops.pack_item_table(W, a.trace_h16)
            del W
            for _ in range(a.reps):
                ops.item_topk(x, im, a.k)
            torch.cuda.synchronize()
            return
        for _ in range(a.reps):
            ops.item_topk(x, W, a.k)
            ops.topk(ops.gemm(x, W, False, True, ldc=ops.pad_ld(V)), a.k, V)
        torch.cuda.synchronize()
        return
    out = []
    for name in a.shapes.split(","):
        for k in (int(v) for v in a.ks.split(",")):
            rec = bench_shape(name, k, a.reps)
            print(json.dumps(rec), flush=True)
            out.append(rec)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), results=out), f, indent=1)


if __name__ == "__main__":
    main()
