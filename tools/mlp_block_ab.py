"""A/B timing of the fused MLP block (csrc/mlp_block.hip) against the composition of the library's own per-layer operators on the
same GPU tensors, on one GPU in one process, the two alternating.

    python tools/mlp_block_ab.py [--reps 200] [--inner 5] [--out profiles/mlp_block_ab.json]

Shapes: T = 20 480 tokens (1024 sessions of 20) with [128 -> 128], [336 -> 128] and [128 -> 256 -> 128]; T = 51 200 with
[256 -> 256].  ReLU, bias, dropout 0.1.  Three figures per shape:
  fwd_train   fused: ops.mlp_stack_fwd(save_acts=True) (one launch, every a_i stored)
              composition: per layer ops.gemm(..., epilogue=EPI_BIAS_RELU) + ops.dropout                  (2 n launches)
  bwd         fused: ops.mlp_stack_bwd_ with every gradient asked for (three launches)
              composition: per layer ops.act_bwd_bias (gate + d b) + ops.gemm_wgrad (d W) + ops.gemm (d input)
  fwd_infer   fused: ops.mlp_stack_fwd (one launch, only the last activation stored); composition: the gemm chain, no dropout
The composition is the comparator, not the code under test; its GEMMs run in the library's default precision mode.  Each sample
times `inner` calls between two device events; the figure is the median over `reps` (>= 200) samples after a warm-up; the spread
of a figure is its interquartile range (min and max are recorded too).  The results of the two are compared before anything is
timed.  `model_step` is one line for a training step (forward, backward, FusedAdam) of the benchmarked model shape (item vocab
100k, d_model 128, 4 layers, 4 heads, L 20, B 1024, MLM, dropout 0.1) without and with mlp_block=MLPBlock([128]).
Fails without a GPU."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(20480, 128, [128]), (20480, 336, [128]), (20480, 128, [256, 128]), (51200, 256, [256])]
P, SEED, OFFSET = 0.1, 1234, 1


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


def _ab(row, what, fused, composition, reps, inner):
    for fn in (fused, composition):           # warm-up
        _timed(fn, inner)
    tf, tc = [], []
    for _ in range(reps):                     # alternating
        tf.append(_timed(fused, inner))
        tc.append(_timed(composition, inner))
    f, c = _stats(tf, "us"), _stats(tc, "us")
    row[what] = {"fused": f, "composition": c,
                 "fused_faster_by_more_than_the_larger_spread": bool(c["us"] - f["us"] > max(f["us_iqr"], c["us_iqr"]))}


def kernels_ab(reps, inner):
    from transformers4rec_amd import ops

    dev = "cuda"
    rows = []
    for T, K0, dims in SHAPES:
        g = torch.Generator().manual_seed(T + K0 + sum(dims))
        n, Ks = len(dims), [K0] + dims[:-1]
        x = torch.randn((T, K0), generator=g).to(dev)
        dout = torch.randn((T, dims[-1]), generator=g).to(dev)
        Ws = [((torch.rand((N, K), generator=g) * 2 - 1) / K ** 0.5).to(dev) for N, K in zip(dims, Ks)]
        bs = [((torch.rand((N,), generator=g) * 2 - 1) / K ** 0.5).to(dev) for N, K in zip(dims, Ks)]
        drop = (P, SEED, OFFSET)
        ctr = [ops.dropout_ctr_hi(OFFSET, i, ops.SITE_MLP_BLOCK) for i in range(n)]
        dW_f, db_f = [torch.zeros_like(w) for w in Ws], [torch.zeros_like(b) for b in bs]
        dW_c, db_c = [torch.zeros_like(w) for w in Ws], [torch.zeros_like(b) for b in bs]

        def fused_fwd():
            return ops.mlp_stack_fwd(x, Ws, bs, True, drop, save_acts=True)

        def comp_fwd(p=P):
            acts, a = [], x
            for i in range(n):
                a = ops.gemm(a, Ws[i], trans_b=True, bias=bs[i], epilogue=ops.EPI_BIAS_RELU)
                if p > 0:
                    a = ops.dropout(a.view(-1), p, SEED, ctr[i]).view(T, dims[i])
                acts.append(a)
            return acts

        acts_f, acts_c = fused_fwd(), comp_fwd()

        def fused_bwd():
            return ops.mlp_stack_bwd_(dout, x, Ws, acts_f, True, drop, dW_f, db_f)

        def comp_bwd(acts=acts_c):
            da = dout
            for i in reversed(range(n)):
                dz = ops.act_bwd_bias(da, acts[i], db_c[i], 1, out=torch.empty_like(da), drop=(P, SEED, ctr[i]))
                ops.gemm_wgrad(dz, acts[i - 1] if i else x, dW_c[i])
                da = ops.gemm(dz, Ws[i])
            return da

        # compared on the SAME activations: an element whose pre-activation is within a rounding of 0 may be positive in one
        # forward and 0 in the other, and one flipped ReLU gate moves a whole row of d x
        dx_f, dx_c = fused_bwd(), comp_bwd(acts_f)
        torch.cuda.synchronize()
        scale = lambda t: max(float(t.abs().max()), 1e-30)      # noqa: E731
        agree = dict(out=float((acts_f[-1] - acts_c[-1]).abs().max()) / scale(acts_c[-1]),
                     dx=float((dx_f - dx_c).abs().max()) / scale(dx_c),
                     dW=max(float((a - b).abs().max()) / scale(b) for a, b in zip(dW_f, dW_c)),
                     db=max(float((a - b).abs().max()) / scale(b) for a, b in zip(db_f, db_c)))
        assert all(v < 1e-3 for v in agree.values()), agree
        row = dict(T=T, K0=K0, dims=dims, relu=True, bias=True, dropout=P, max_rel_diff=agree)
        _ab(row, "fwd_train", fused_fwd, comp_fwd, reps, inner)
        _ab(row, "bwd", fused_bwd, comp_bwd, reps, inner)
        for g0 in dW_c + db_c:                       # what the timed backward calls accumulated is dropped
            g0.zero_()
        _ab(row, "fwd_infer", lambda: ops.mlp_stack_fwd(x, Ws, bs, True), lambda: comp_fwd(0.0), reps, inner)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def model_step(steps=30, warmup=10):
    import transformers4rec_amd as tr

    V, D, L, B = 100_000, 128, 20, 1024
    out = {}
    for name, mlp in (("without", None), ("with_mlp_block_128", tr.MLPBlock([D]))):
        torch.manual_seed(0)
        feats = tr.TabularSequenceFeatures.from_schema(tr.session_schema(V, L), max_sequence_length=L, masking="mlm",
                                                       embedding_dim_default=D)
        cfg = tr.XLNetConfig.build(D, 4, 4, total_seq_length=L, dropout=0.1)
        model = tr.Model(feats, tr.TransformerBlock(cfg, masking=feats.masking), tr.NextItemPredictionTask(weight_tying=True),
                         mlp_block=mlp).to("cuda").train()
        dense, tables = tr.flatten_model(model)
        opt = tr.FusedAdam([dense, tables], lr=1e-3)
        ids = torch.randint(1, V + 1, (B, L), generator=torch.Generator().manual_seed(1)).to("cuda")

        def step():
            model({"item_id": ids}, training=True)["loss"].backward()
            opt.step()

        for _ in range(warmup):
            step()
        ms = [_timed(step, 1) / 1e3 for _ in range(steps)]
        out[name] = _stats(ms, "ms")
        del model, opt, dense, tables
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("mlp_block_ab: no GPU visible; a timing needs one")
    reps, inner = _arg("--reps", 200, int), _arg("--inner", 5, int)
    path = _arg("--out", os.path.join(ROOT, "profiles", "mlp_block_ab.json"), str)
    assert reps >= 200, "each figure is the median over at least 200 samples"
    res = dict(device=torch.cuda.get_device_name(0), reps=reps, inner=inner,
               method="median over reps of device-event time per call, fused and composition alternating in one process; "
                      "spread = interquartile range", kernels=kernels_ab(reps, inner), model_step=model_step())
    print(json.dumps(res["model_step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
