#!/usr/bin/env python
"""The fused gather + projection of a pretrained-embedding feature (ops.pretrained_proj_fwd / _bwd, csrc/pretrained_proj.hip)
against what a user could do before it existed, in the same process on the same box: image[ids].float() -> ops.gemm (bias
epilogue) -> LayerNorm, and backward LayerNorm backward -> bias column sum -> ops.gemm_wgrad.  T = 20 480 tokens (BASELINE
configs[1]), V = 100 000, E in {384, 768}, P = 64, LayerNorm on.  The legs are interleaved, timed with device events; median
(minimum) microseconds, the bytes each leg has to move by its algorithm (computed from the shapes below) and the box's copy
ceiling (the float4 copy kernel of tools/t4r_tools.hip over 256 MiB).

    python tools/pretrained_bench.py --out profiles/pretrained_proj_ab.json
"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--tokens", type=int, default=20480)
ap.add_argument("--rows", type=int, default=100000)
ap.add_argument("--widths", default="384,768")
ap.add_argument("--proj", type=int, default=64)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import t4r_tools  # noqa: E402
from transformers4rec_amd import ops  # noqa: E402

DEV = "cuda"
T, V, P = args.tokens, args.rows, args.proj


def timed(legs, reps):
    for fn in legs.values():
        fn()
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


def copy_ceiling():
    n = 256 << 20
    a, b = torch.empty(n, dtype=torch.uint8, device=DEV), torch.empty(n, dtype=torch.uint8, device=DEV)
    t = timed({"copy": lambda: t4r_tools.copy(b, a)}, 20)["copy"]
    return 2 * n / (statistics.median(t) * 1e-6) / 1e12       # TB/s, read + write


ceiling = copy_ceiling()
rows = []
g = torch.Generator(device=DEV).manual_seed(0)
for E in (int(e) for e in args.widths.split(",")):
    image = ops.pack_item_table(torch.randn((V, E), device=DEV, generator=g), "fp16")
    ids = torch.randint(0, V, (T,), device=DEV, generator=g)
    lin = torch.nn.Linear(E, P).to(DEV)
    W, b = lin.weight.detach(), lin.bias.detach()
    gamma, beta = torch.ones(P, device=DEV), torch.zeros(P, device=DEV)
    dY = torch.randn((T, P), device=DEV, generator=g)
    grads = [torch.zeros_like(W), torch.zeros_like(b), torch.zeros_like(gamma), torch.zeros_like(beta)]
    state = {}

    def fused_fwd():
        state["f"] = ops.pretrained_proj_fwd(image, ids, W, b, gamma, beta)

    def fused_bwd():
        _o, xhat, rstd = state["f"]
        ops.pretrained_proj_bwd(dY, image, ids, gamma, xhat, rstd, *grads)

    def dense_fwd():
        x = image[ids].float()
        z = ops.gemm(x, W, False, True, bias=b, epilogue=ops.EPI_BIAS)
        state["d"] = (x, z) + tuple(ops.add_layernorm_fwd(z, None, gamma, beta, 1e-5))

    def dense_bwd():
        x, z, _y, mean, rstd = state["d"]
        dz = ops.add_layernorm_bwd(z, None, gamma, mean, rstd, dY, grads[2], grads[3])
        ops.colsum_(dz, grads[1])
        ops.gemm_wgrad(dz, x, grads[0])

    def dense_bwd_regather():       # the composition when the [T, E] fp32 rows are not kept from the forward
        x = image[ids].float()
        _x, z, _y, mean, rstd = state["d"]
        dz = ops.add_layernorm_bwd(z, None, gamma, mean, rstd, dY, grads[2], grads[3])
        ops.colsum_(dz, grads[1])
        ops.gemm_wgrad(dz, x, grads[0])

    fused_fwd()
    dense_fwd()
    torch.cuda.synchronize()
    agree = float((state["f"][0] - state["d"][2]).abs().max())
    t = timed(dict(fused_fwd=fused_fwd, dense_fwd=dense_fwd, fused_bwd=fused_bwd, dense_bwd=dense_bwd,
                   dense_bwd_regather=dense_bwd_regather), args.reps)
    ldp = image.stride(0)
    row16, row32, out32 = T * ldp * 2, T * E * 4, T * P * 4
    # bytes by the algorithm: fused forward reads the 16-bit rows and writes out, xhat; the composition also writes and reads the
    # fp32 rows (16-bit read, fp32 write, fp32 read by the GEMM, z written and read, out written)
    nbytes = dict(fused_fwd=row16 + 2 * out32, dense_fwd=row16 + 2 * row32 + 3 * out32,
                  fused_bwd=row16 + 4 * out32, dense_bwd=row32 + 4 * out32, dense_bwd_regather=row16 + 2 * row32 + 4 * out32)
    row = dict(T=T, V=V, E=E, P=P, layer_norm=True, max_abs_difference_fused_vs_dense=agree)
    for name, v in t.items():
        med = statistics.median(v)
        row[name + "_us_median"] = round(med, 1)
        row[name + "_us_min"] = round(min(v), 1)
        row[name + "_MB"] = round(nbytes[name] / 1e6, 1)
        row[name + "_share_of_copy_ceiling"] = round(nbytes[name] / (med * 1e-6) / 1e12 / ceiling, 3)
    row["fwd_speedup"] = round(row["dense_fwd_us_median"] / row["fused_fwd_us_median"], 2)
    row["bwd_speedup"] = round(row["dense_bwd_us_median"] / row["fused_bwd_us_median"], 2)
    rows.append(row)
    print(json.dumps(row), flush=True)
res = dict(tool="tools/pretrained_bench.py", reps=args.reps, device=torch.cuda.get_device_name(0),
           copy_ceiling_TBps=round(ceiling, 2), rows=rows)
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
