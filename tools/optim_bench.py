"""What global-norm clipping + AdamW cost on top of the plain fused Adam step, at the bucket sizes of BASELINE configs[1]
(tables 100 001 x 128, dense ~ 0.85 M floats).

One process, device events, legs alternated inside every iteration (so that a drift of the box hits all of them alike):

  plain    the step FusedAdam() runs: t4r_adam_step_amax (tables) + t4r_adam_step (dense)                      2 launches
  clipped  FusedAdam(weight_decay=0.01, decoupled_weight_decay=True, max_grad_norm=1.0):
           t4r_grad_sumsq x 2, t4r_grad_clip_coef, t4r_adamw_step x 2                                             5 launches
  sumsq    the two t4r_grad_sumsq launches alone: 4 bytes per gradient element (sumsq_tables / sumsq_dense: each launch by
           itself; coef: the one-workgroup t4r_grad_clip_coef, i.e. what a launch costs when it has nothing to stream), against
  copy     the float4 copy kernel of tools/t4r_tools.hip over a buffer of the gradients' size (read + write bytes / time; plain
           and non-temporal, the better one): what a kernel that only moves bytes reaches on this box

    python tools/optim_bench.py [--iters 200] [--warmup 20] [--out profiles/optim_clip_ab.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_TABLES = 100_001 * 128
N_DENSE = 850_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_clip_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench needs the GPU: a CPU run measures nothing")
    import t4r_tools
    from transformers4rec_amd import ops

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    buckets = []
    for n in (N_TABLES, N_DENSE):
        p = 0.05 * torch.randn(n, generator=g, device=dev)
        buckets.append(dict(p=p, g=torch.randn(n, generator=g, device=dev), m=torch.zeros_like(p), v=torch.zeros_like(p)))
    amax_part = torch.zeros(1024, device=dev)
    part = torch.zeros(sum(ops.grad_sumsq_parts(b["p"].numel()) for b in buckets), device=dev, dtype=torch.float64)
    out2 = torch.zeros(2, device=dev)
    cp_src = torch.randn(N_TABLES + N_DENSE, generator=g, device=dev)
    cp_dst = torch.empty_like(cp_src)
    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    step = [0]

    def plain():
        t, d = buckets
        ops.adam_step_amax_(t["p"], t["g"], t["m"], t["v"], step[0], 0, N_TABLES, amax_part, weight_decay=0.0, **hp)
        ops.adam_step_(d["p"], d["g"], d["m"], d["v"], step[0], weight_decay=0.0, **hp)

    def sumsq():
        n = 0
        for b in buckets:
            n += ops.grad_sumsq_(b["g"], part[n:])
        return n

    def clipped():
        n = sumsq()
        ops.grad_clip_coef_(part, n, 1.0, 1.0, out2)
        for k, b in enumerate(buckets):
            ops.adamw_step_(b["p"], b["g"], b["m"], b["v"], step[0], weight_decay=0.01, decoupled=True, clip_coef=out2[1:],
                            amax=(0, N_TABLES, amax_part) if k == 0 else None, **hp)

    legs = {"plain": plain, "clipped": clipped, "sumsq": sumsq,
            "sumsq_tables": lambda: ops.grad_sumsq_(buckets[0]["g"], part), "sumsq_dense": lambda: ops.grad_sumsq_(buckets[1]["g"], part),
            "coef": lambda: ops.grad_clip_coef_(part, part.numel(), 1.0, 1.0, out2),
            "copy_float4": lambda: t4r_tools.copy(cp_dst, cp_src, mode=0),
            "copy_float4_nt": lambda: t4r_tools.copy(cp_dst, cp_src, mode=1)}
    times = {k: [] for k in legs}
    order = list(legs)
    for it in range(args.warmup + args.iters):
        step[0] += 1
        for b in buckets:                    # every step zeroes the gradients: give each iteration real ones again (untimed; the
                                             # later legs of an iteration see zeros, and no leg's time depends on the values)
            b["g"].normal_(generator=g)
        for name in order[it % 2:] + order[:it % 2]:          # alternate which of plain / clipped goes first
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            legs[name]()
            e1.record()
            e1.synchronize()
            if it >= args.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    for b in buckets:                        # one more clipped step on real gradients: the norm and coefficient the record shows
        b["g"].normal_(generator=g)
    step[0] += 1
    clipped()
    torch.cuda.synchronize()

    def stats(v):
        v = sorted(v)
        return {"median_us": round(statistics.median(v), 2), "p10_us": round(v[len(v) // 10], 2), "p90_us": round(v[len(v) * 9 // 10], 2)}

    n_el = N_TABLES + N_DENSE
    res = {k: stats(v) for k, v in times.items()}
    copy_best = min(res["copy_float4"]["median_us"], res["copy_float4_nt"]["median_us"])
    copy_rate = 2.0 * 4 * n_el / (copy_best * 1e-6)
    sumsq_rate = 4.0 * n_el / (res["sumsq"]["median_us"] * 1e-6)
    record = {
        "tool": "tools/optim_bench.py", "device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup,
        "elements": {"tables": N_TABLES, "dense": N_DENSE},
        "timing": "device events around each leg, one process, legs alternated within every iteration; microseconds",
        "legs": res,
        "clipped_minus_plain_us": round(res["clipped"]["median_us"] - res["plain"]["median_us"], 2),
        "sumsq_bytes": 4 * n_el, "sumsq_GBps": round(sumsq_rate / 1e9, 1),
        "sumsq_tables_GBps": round(4.0 * N_TABLES / (res["sumsq_tables"]["median_us"] * 1e-6) / 1e9, 1),
        "sumsq_tables_fraction_of_copy_ceiling": round(4.0 * N_TABLES / (res["sumsq_tables"]["median_us"] * 1e-6) / copy_rate, 3),
        "copy_ceiling_GBps": round(copy_rate / 1e9, 1), "copy_ceiling_note": "read + write bytes of the better float4 copy form over its median",
        "sumsq_fraction_of_copy_ceiling": round(sumsq_rate / copy_rate, 3),
        "norm": float(out2[0]), "coef": float(out2[1]),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
