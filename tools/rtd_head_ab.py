"""A/B timing of the fused replaced-token-detection head (csrc/rtd_head.hip) against the composition of existing operators on
the same GPU tensors, on one GPU in one process, the two alternating.

    python tools/rtd_head_ab.py [--reps 200] [--inner 5] [--out profiles/rtd_head_ab.json] [--no-step]

At (T, D) = (20 480, 128) (configs[1]: 1024 sessions of 20) and (51 200, 256), erf-GELU, 70 % of the tokens active:
  fused        ops.rtd_head_fwd + ops.rtd_head_bwd_                                                      (2 + 3 launches)
  composition  ops.gemm with its bias epilogue (backward: ops.gemm, ops.gemm_wgrad, a column sum) -> torch gelu -> a row dot
               with w2 + b2 -> binary_cross_entropy_with_logits over the active rows, backward by autograd
The composition is the comparator, not the code under test.  Each sample times `inner` forward + backward pairs between two
device events; the figure is the median over `reps` (>= 200) samples after a warm-up; the spread of a figure is its
interquartile range (min and max are recorded too).  The losses and gradients of the two are compared before anything is
timed.  Unless --no-step, one training step (forward + backward + fused Adam) of a small config (1 000 items, d_model 64,
2 layers, 256 sessions of 20) is recorded as plain MLM and as RTD (generator + discriminator of that size, shared item table).
Fails without a GPU."""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(20480, 128), (51200, 256)]


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


class _LinearBias(torch.autograd.Function):
    """x W^T + b through the package's GEMM (bias in the epilogue), its backward through the package's GEMMs"""

    @staticmethod
    def forward(ctx, x, W, b):
        from transformers4rec_amd import ops

        ctx.save_for_backward(x, W)
        return ops.gemm(x, W, False, True, bias=b, epilogue=ops.EPI_BIAS)

    @staticmethod
    def backward(ctx, da):
        from transformers4rec_amd import ops

        x, W = ctx.saved_tensors
        da = da.contiguous()
        dW = torch.zeros_like(W)
        ops.gemm_wgrad(da, x, dW)
        return ops.gemm(da, W, False, False), dW, da.sum(0)


def kernels_ab(reps, inner):
    from transformers4rec_amd import ops

    dev = "cuda"
    rows = []
    for T, D in SHAPES:
        g = torch.Generator().manual_seed(T + D)
        x = torch.randn((T, D), generator=g).to(dev)
        W1 = (torch.randn((D, D), generator=g) / D ** 0.5).to(dev)
        b1 = (torch.randn((D,), generator=g) * 0.1).to(dev)
        w2 = (torch.randn((D,), generator=g) / D ** 0.5).to(dev)
        b2 = torch.full((1,), 0.3, device=dev)
        label = (torch.rand((T,), generator=g) < 0.15).to(dev)
        active = (torch.rand((T,), generator=g) < 0.7).to(dev)
        target = label.float()[active]
        one = torch.ones(1, device=dev)
        grads = [torch.zeros_like(t) for t in (W1, b1, w2, b2)]
        xa, Wa, b1a, w2a, b2a = (t.clone().requires_grad_(True) for t in (x, W1, b1, w2, b2))

        def fused():
            z, n, loss = ops.rtd_head_fwd(x, active, label, W1, b1, w2, b2, 0)
            return loss, ops.rtd_head_bwd_(one, x, active, label, z, n, W1, b1, w2, 0, *grads)

        def composition():
            for t in (xa, Wa, b1a, w2a, b2a):
                t.grad = None
            h = F.gelu(_LinearBias.apply(xa, Wa, b1a))
            z = h @ w2a + b2a
            loss = F.binary_cross_entropy_with_logits(z[active], target)
            loss.backward()
            return loss, xa.grad

        for t in grads:
            t.zero_()
        (la, dxa), (lb, dxb) = fused(), composition()
        torch.cuda.synchronize()
        agree = dict(loss=float((la.view(()) - lb.detach()).abs()), dx=float((dxa - dxb).abs().max()),
                     d_W1=float((grads[0] - Wa.grad).abs().max()), d_w2=float((grads[2] - w2a.grad).abs().max()))
        assert agree["loss"] < 1e-5 and agree["dx"] < 1e-6 and agree["d_W1"] < 1e-4 and agree["d_w2"] < 1e-4, agree
        for fn in (fused, composition):           # warm-up
            _timed(fn, inner)
        tf, tc = [], []
        for _ in range(reps):                     # alternating
            tf.append(_timed(fused, inner))
            tc.append(_timed(composition, inner))
        row = dict(T=T, D=D, act="gelu", max_abs_diff=agree)
        row.update({"fused_" + k: v for k, v in _stats(tf, "us").items()})
        row.update({"composition_" + k: v for k, v in _stats(tc, "us").items()})
        row["fused_faster_by_more_than_the_larger_spread"] = bool(
            row["composition_us"] - row["fused_us"] > max(row["fused_us_iqr"], row["composition_us_iqr"]))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def training_step(reps):
    """ms per training step of one small config as plain MLM and as RTD"""
    import transformers4rec_amd as tr

    V, D, L, B = 1000, 64, 20, 256
    schema = tr.session_schema(V, L)

    def feats(masking):
        return tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=L, masking=masking, aggregation="concat",
                                                      embedding_dims={"item_id": D})

    runs, out = {}, {}
    for form in ("mlm", "rtd"):
        torch.manual_seed(0)
        cfg = tr.XLNetConfig.build(D, 4, 2, total_seq_length=L, dropout=0.1)
        model = cfg.to_torch_model(feats("mlm" if form == "mlm" else "rtd"), tr.NextItemPredictionTask(weight_tying=True))
        if form == "rtd":
            model = tr.RTDModel(model, feats(None), tr.TransformerBlock(cfg))
        model = model.to("cuda").train()
        dense, tables = tr.flatten_model(model)
        opt = tr.FusedAdam([dense, tables], lr=1e-3)
        batches = [{k: v.to("cuda") for k, v in tr.random_data_from_schema(schema, B, L, seed=100 + i).items()} for i in range(4)]

        def step(i, model=model, opt=opt, batches=batches):
            opt.zero_grad()
            model(batches[i % 4], training=True)["loss"].backward()
            opt.step()

        for i in range(8):
            step(i)
        torch.cuda.synchronize()
        runs[form], out[form] = step, []
    for r in range(reps):
        for form, step in runs.items():
            out[form].append(_timed(lambda: step(r), 5) / 1e3)
    return {form: _stats(v, "step_ms") for form, v in out.items()}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("rtd_head_ab: no GPU visible; a timing needs one")
    reps, inner = _arg("--reps", 200, int), _arg("--inner", 5, int)
    path = _arg("--out", os.path.join(ROOT, "profiles", "rtd_head_ab.json"), str)
    assert reps >= 200, "each figure is the median over at least 200 samples"
    res = dict(device=torch.cuda.get_device_name(0), reps=reps, inner=inner,
               method="median over reps of device-event time per forward + backward pair, fused and composition alternating in "
                      "one process; spread = interquartile range", kernels=kernels_ab(reps, inner))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    if "--no-step" not in sys.argv:
        res["training_step_small_config"] = training_step(max(40, reps // 5))
        print(json.dumps(res["training_step_small_config"]), flush=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
