"""A/B timing of the fused post-context fusion (csrc/post_fusion.hip) against the torch composition of the same chain on the same
GPU tensors, on one GPU in one process, the two alternating.

    python tools/post_fusion_ab.py [--reps 200] [--inner 5] [--out profiles/post_fusion_ab.json]

At (T, D, C) = (20 480, 128, 64) and (20 480, 128, 256) (1024 sessions of 20), elementwise-mul, a sequence-level [B, L, C] and a
session-level [B, C] context:
  fused        ops.post_fusion_fwd + ops.post_fusion_bwd_ with every gradient asked for              (1 + 3 launches)
  composition  the reference's chain (transformers4rec/torch/experimental.py:85-97): unsqueeze + repeat of a 2-D context,
               F.linear, torch.multiply(seq, 1.0 + p), backward by autograd
The composition is the comparator, not the code under test.  Each sample times `inner` forward + backward pairs between two
device events; the figure is the median over `reps` (>= 200) samples after a warm-up; the spread of a figure is its
interquartile range (min and max are recorded too).  The outputs and gradients of the two are compared before anything is
timed.  Fails without a GPU."""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(1024, 20, 128, 64), (1024, 20, 128, 256)]


def _arg(name, default, cast):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner        # microseconds per call


def _stats(v, unit):
    q = statistics.quantiles(v, n=4)
    return {f"{unit}": statistics.median(v), f"{unit}_iqr": q[2] - q[0], f"{unit}_min": min(v), f"{unit}_max": max(v)}


def kernels_ab(reps, inner):
    from transformers4rec_amd import ops

    dev = "cuda"
    rows = []
    for B, L, D, C in SHAPES:
        for session in (False, True):
            g = torch.Generator().manual_seed(B + D + C + int(session))
            seq = torch.randn((B, L, D), generator=g).to(dev)
            ctx = torch.randn((B, C) if session else (B, L, C), generator=g).to(dev)
            dout = torch.randn((B, L, D), generator=g).to(dev)
            W = ((torch.rand((D, C), generator=g) * 2 - 1) / C ** 0.5).to(dev)
            b = ((torch.rand((D,), generator=g) * 2 - 1) / C ** 0.5).to(dev)
            d_w, d_b = torch.zeros_like(W), torch.zeros_like(b)
            sa, ca, Wa, ba = (t.clone().requires_grad_(True) for t in (seq, ctx, W, b))

            def fused():
                out = ops.post_fusion_fwd(seq, ctx, W, b, ops.FUSION_MUL)
                return out, ops.post_fusion_bwd_(dout, seq, ctx, W, b, ops.FUSION_MUL, d_w, d_b)

            def composition():
                for t in (sa, ca, Wa, ba):
                    t.grad = None
                x = ca.unsqueeze(1).repeat(1, L, 1) if session else ca
                out = torch.multiply(sa, 1.0 + F.linear(x, Wa, ba))
                out.backward(dout)
                return out, (sa.grad, ca.grad)

            d_w.zero_()
            d_b.zero_()
            (oa, (dsa, dca)), (ob, (dsb, dcb)) = fused(), composition()
            torch.cuda.synchronize()
            scale = lambda t: max(float(t.abs().max()), 1e-30)      # noqa: E731
            agree = dict(out=float((oa - ob.detach()).abs().max()) / scale(ob), dseq=float((dsa - dsb).abs().max()) / scale(dsb),
                         dctx=float((dca - dcb).abs().max()) / scale(dcb), d_w=float((d_w - Wa.grad).abs().max()) / scale(Wa.grad),
                         d_b=float((d_b - ba.grad).abs().max()) / scale(ba.grad))
            assert all(v < 1e-4 for v in agree.values()), agree
            for fn in (fused, composition):           # warm-up
                _timed(fn, inner)
            tf, tc = [], []
            for _ in range(reps):                     # alternating
                tf.append(_timed(fused, inner))
                tc.append(_timed(composition, inner))
            row = dict(T=B * L, L=L, D=D, C=C, context="session" if session else "sequence", aggregation="elementwise-mul",
                       max_rel_diff=agree)
            row.update({"fused_" + k: v for k, v in _stats(tf, "us").items()})
            row.update({"composition_" + k: v for k, v in _stats(tc, "us").items()})
            row["fused_faster_by_more_than_the_larger_spread"] = bool(
                row["composition_us"] - row["fused_us"] > max(row["fused_us_iqr"], row["composition_us_iqr"]))
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def main():
    if not torch.cuda.is_available():
        raise SystemExit("post_fusion_ab: no GPU visible; a timing needs one")
    reps, inner = _arg("--reps", 200, int), _arg("--inner", 5, int)
    path = _arg("--out", os.path.join(ROOT, "profiles", "post_fusion_ab.json"), str)
    assert reps >= 200, "each figure is the median over at least 200 samples"
    res = dict(device=torch.cuda.get_device_name(0), reps=reps, inner=inner,
               method="median over reps of device-event time per forward + backward pair, fused and composition alternating in "
                      "one process; spread = interquartile range", kernels=kernels_ab(reps, inner))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
