"""A/B timing of the fused GRU block (csrc/gru.hip) against torch.nn.GRU(batch_first=True) on the same GPU tensors, on one GPU in
one process, the two alternating.  torch.nn.GRU is what a user of the reference runs today; there is no GRU at the parent commit.

    python tools/gru_ab.py [--reps 200] [--inner 5] [--out profiles/gru_ab.json]

Shapes (B, L, K0 = H, layers): (1024, 20, 128, 1), (1024, 20, 64, 2), (256, 100, 128, 1).  Two figures per shape:
  fwd_train   fused: ops.gru_fwd(save=True);  torch: gru(x) with gradients enabled
  fwd_bwd     fused: ops.gru_fwd(save=True) + ops.gru_bwd_ with every gradient asked for;  torch: gru(x)[0].backward(dout)
The two share their parameter values; their outputs are compared before anything is timed.  Each sample times `inner` calls
between two device events; the figure is the median over `reps` (>= 200) samples after a warm-up; the spread of a figure is its
interquartile range (min and max are recorded too).  `model_step` is one training step (forward, backward, FusedAdam) of
Model(item-only CLM inputs, MLPBlock([128]), GRUBlock(128, 128)) at item vocabulary 100k, L 20, B 1024.  `workgroups` is the
recurrence kernels' grid at the shape against the chip's 256 CUs.  Fails without a GPU."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(1024, 20, 128, 1), (1024, 20, 64, 2), (256, 100, 128, 1)]


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


def _ab(row, what, fused, other, reps, inner):
    for fn in (fused, other):                 # warm-up
        for _ in range(3):
            _timed(fn, inner)
    tf, tc = [], []
    for _ in range(reps):                     # alternating
        tf.append(_timed(fused, inner))
        tc.append(_timed(other, inner))
    f, c = _stats(tf, "us"), _stats(tc, "us")
    row[what] = {"fused": f, "torch_nn_gru": c,
                 "fused_faster_by_more_than_the_larger_spread": bool(c["us"] - f["us"] > max(f["us_iqr"], c["us_iqr"]))}


def main():
    import transformers4rec_amd as tr
    from transformers4rec_amd import ops

    reps, inner = max(200, _arg("--reps", 200, int)), _arg("--inner", 5, int)
    out_path = _arg("--out", os.path.join(ROOT, "profiles", "gru_ab.json"), str)
    dev = "cuda"
    res = {"device": torch.cuda.get_device_name(0), "reps": reps, "inner": inner, "shapes": []}
    for B, L, H, n in SHAPES:
        torch.manual_seed(0)
        gru = torch.nn.GRU(H, H, num_layers=n, batch_first=True).to(dev)
        blk = tr.Block(gru, [None, L, H]).to(dev)
        x = torch.randn(B, L, H, device=dev)
        dout = torch.randn(B, L, H, device=dev)
        Wi, Wh, bi, bh = blk._params()
        xg = x.clone().requires_grad_()
        want = gru(xg)[0]
        got, saved = ops.gru_fwd(x, Wi, Wh, bi, bh, None, ops.NO_DROP, save=True)
        row = {"B": B, "L": L, "K0": H, "H": H, "layers": n, "workgroups": (B + 15) // 16, "cus": 256,
               "max_abs_diff_vs_torch": float((got - want.detach()).abs().max())}
        grads = [[torch.zeros_like(t) for t in ts] for ts in (Wi, Wh, bi, bh)]

        def fused_fwd():
            ops.gru_fwd(x, Wi, Wh, bi, bh, None, ops.NO_DROP, save=True)

        def torch_fwd():
            gru(xg)

        def fused_fb():
            o, s = ops.gru_fwd(x, Wi, Wh, bi, bh, None, ops.NO_DROP, save=True)
            ops.gru_bwd_(dout, x, Wi, Wh, o, s, None, ops.NO_DROP, *grads)

        def torch_fb():
            gru(xg)[0].backward(dout)

        _ab(row, "fwd_train", fused_fwd, torch_fwd, reps, inner)
        _ab(row, "fwd_bwd", fused_fb, torch_fb, reps, inner)
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
    # one training step of a model with the block
    V, L, B, D = 100000, 20, 1024, 128
    torch.manual_seed(0)
    feats = tr.TabularSequenceFeatures.from_schema(tr.session_schema(V, L), max_sequence_length=L, masking="clm",
                                                   aggregation="concat", embedding_dims={"item_id": D})
    model = tr.Model(feats, tr.GRUBlock(D, D), tr.NextItemPredictionTask(weight_tying=True), mlp_block=tr.MLPBlock([D])).to(dev).train()
    dense, tables = tr.flatten_model(model)
    opt = tr.FusedAdam([b for b in (dense, tables) if b is not None], lr=1e-3)
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(2, L + 1, (B,), generator=g)
    ids = (torch.randint(1, V + 1, (B, L), generator=g) * (torch.arange(L)[None] < lens[:, None])).to(dev)

    def step():
        model({"item_id": ids}, training=True)["loss"].backward()
        opt.step()

    for _ in range(10):
        _timed(step, 1)
    res["model_step"] = dict(_stats([_timed(step, 1) for _ in range(reps)], "us"), B=B, L=L, V=V, d_model=D,
                             body="MLPBlock([128]) + GRUBlock(128, 128), CLM, tied head, FusedAdam")
    print(json.dumps(res["model_step"]), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
