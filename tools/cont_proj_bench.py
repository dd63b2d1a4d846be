"""A/B timing of the first layer of `continuous_projection` (csrc/cont_proj.hip) against the same result composed from the
operators the package had before it, on one GPU in one process, the two alternating.

    python tools/cont_proj_bench.py [--reps 30] [--inner 20] [--out profiles/cont_proj_ab.json] [--no-step]

At the configs[2] token count, T = 1024 sessions x 20 positions = 20 480, for C in {2, 8} columns and P in {64, 128} units:
  fused     ops.cont_proj_fwd + ops.cont_proj_bwd_                       (1 + 2 launches, no [T, C] operand)
  composed  torch.stack of the columns -> ops.gemm(EPI_BIAS_RELU); ops.act_bwd_bias -> ops.gemm_wgrad
Each repetition times `inner` forward + backward pairs between two device events; the figure is the median over the
repetitions, after a warm-up of every shape.  The outputs and gradients of the two are compared before anything is timed.
Unless --no-step, one training step (forward + backward + fused Adam) of the configs[2] model is also recorded with its two
continuous features soft-embedded (as benchmarked) and projected (continuous_projection=64)."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, L = 1024, 20
SHAPES = [(2, 64), (2, 128), (8, 64), (8, 128)]


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


def first_layer_ab(reps, inner):
    from transformers4rec_amd import ops

    dev = "cuda"
    rows = []
    for C, P in SHAPES:
        g = torch.Generator().manual_seed(C * 1000 + P)
        xs = [torch.rand((B, L), generator=g).to(dev) for _ in range(C)]
        flags = [False] * C
        W = ((torch.rand((P, C), generator=g) * 2 - 1) / C ** 0.5).to(dev)
        b = ((torch.rand((P,), generator=g) * 2 - 1) / C ** 0.5).to(dev)
        dY = torch.randn((B * L, P), generator=g).to(dev)
        gW = [torch.zeros_like(W) for _ in range(2)]
        gb = [torch.zeros_like(b) for _ in range(2)]

        def fused():
            y = ops.cont_proj_fwd(xs, flags, W, b)
            ops.cont_proj_bwd_(dY, 0, xs, flags, W, b, gW[0], gb[0])
            return y

        def composed():
            X = torch.stack(xs, dim=-1).view(B * L, C)
            y = ops.gemm(X, W, False, True, bias=b, epilogue=ops.EPI_BIAS_RELU)
            d = ops.act_bwd_bias(dY, y, gb[1], 1, out=torch.empty_like(dY))
            ops.gemm_wgrad(d, X, gW[1])
            return y

        ya, yb = fused(), composed()
        torch.cuda.synchronize()
        agree = dict(y=float((ya - yb).abs().max()), d_w=float((gW[0] - gW[1]).abs().max() / gW[1].abs().max()),
                     d_b=float((gb[0] - gb[1]).abs().max() / gb[1].abs().max()))
        assert agree["y"] < 1e-4 and agree["d_w"] < 1e-4 and agree["d_b"] < 1e-4, agree
        for fn in (fused, composed):            # warm-up
            _timed(fn, inner)
        tf, tc = [], []
        for _ in range(reps):                   # alternating
            tf.append(_timed(fused, inner))
            tc.append(_timed(composed, inner))
        T = B * L
        rows.append(dict(C=C, P=P, T=T, fused_us=statistics.median(tf), composed_us=statistics.median(tc),
                         fused_us_min=min(tf), fused_us_max=max(tf), composed_us_min=min(tc), composed_us_max=max(tc),
                         forward_bytes=T * (4 * C + 4 * P), backward_bytes=T * (4 * C + 4 * P), max_abs_diff=agree))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def training_step(reps):
    """ms per training step of the configs[2] model, continuous features soft-embedded vs projected to 64"""
    import transformers4rec_amd as tr

    V, D, cats, conts = 100_000, 128, (("category", 1000), ("brand", 100), ("dow", 10)), ("price", "age")
    schema = tr.session_schema(V, L, cats, conts)
    out = {}
    runs = {}
    for form, kw in (("soft_embeddings", dict(continuous_soft_embeddings=True)), ("continuous_projection_64", dict(continuous_projection=64))):
        torch.manual_seed(0)
        inputs = tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=L, masking="mlm", aggregation="concat", d_output=D,
                                                        embedding_dims={"item_id": D}, embedding_dim_default=64, **kw)
        model = tr.XLNetConfig.build(D, 4, 4, total_seq_length=L, dropout=0.3).to_torch_model(
            inputs, tr.NextItemPredictionTask(weight_tying=True)).to("cuda")
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
        runs[form] = step
        out[form] = []
    for r in range(reps):
        for form, step in runs.items():
            out[form].append(_timed(lambda: step(r), 5) / 1e3)
    return {form: dict(step_ms=statistics.median(v), step_ms_min=min(v), step_ms_max=max(v)) for form, v in out.items()}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("cont_proj_bench: no GPU visible; a timing needs one")
    reps, inner = _arg("--reps", 30, int), _arg("--inner", 20, int)
    path = _arg("--out", os.path.join(ROOT, "profiles", "cont_proj_ab.json"), str)
    assert reps >= 20
    res = dict(device=torch.cuda.get_device_name(0), reps=reps, inner=inner, method="median over reps of device-event time per "
               "forward + backward pair, fused and composed alternating in one process", first_layer=first_layer_ab(reps, inner))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    if "--no-step" not in sys.argv:
        res["training_step_configs2"] = training_step(reps)
        print(json.dumps(res["training_step_configs2"]), flush=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
