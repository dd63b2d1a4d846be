"""A/B timing of the fused session-level task kernels (csrc/seq_task.hip) against the op chain the reference's tasks run on the
same GPU tensors, on one GPU in one process, the two alternating.

    python tools/seq_task_bench.py [--reps 200] [--inner 5] [--out profiles/seq_task_ab.json] [--no-step]

At B = 1024 sessions and (L, D) in {(20, 128) (configs[1]), (50, 256), (100, 512)}, for the three summaries, binary
classification (Linear without bias, sigmoid, BCELoss) and regression (Linear with bias, MSELoss):
  fused   ops.seq_task_fwd + ops.seq_task_bwd_                                      (2 + 2 launches)
  chain   x.mean(1) | x[:, 0] | x[:, -1] -> F.linear -> sigmoid -> squeeze -> BCELoss / MSELoss, backward by autograd
Each sample times `inner` forward + backward pairs between two device events; the figure is the median over `reps` (>= 200)
samples, after a warm-up of every shape; the spread of a figure is its interquartile range (min and max are recorded too).  The
losses and gradients of the two are compared before anything is timed.  Unless --no-step, one training step (forward + backward
+ fused Adam) of the configs[1] model (100k items, d_model 128, 4 layers, CLM so that no draw differs) is recorded with its
next-item task alone and with a binary `mean` task added.  Fails without a GPU."""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B = 1024
SHAPES = [(20, 128), (50, 256), (100, 512)]


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
    for L, D in SHAPES:
        g = torch.Generator().manual_seed(L * 1000 + D)
        x = torch.randn((B, L, D), generator=g).to(dev)
        for kind in ("binary", "regression"):
            w = ((torch.rand((1, D), generator=g) * 2 - 1) / D ** 0.5).to(dev)
            b = None if kind == "binary" else torch.zeros(1, device=dev)
            t = (torch.randint(0, 2, (B,), generator=g).float() if kind == "binary" else torch.randn((B,), generator=g)).to(dev)
            act, lk = (ops.ACT_SIGMOID, ops.LOSS_BCE) if kind == "binary" else (ops.ACT_NONE, ops.LOSS_MSE)
            one = torch.ones(1, device=dev)
            for summary in ("first", "last", "mean"):
                mode = ops.SUMMARY[summary]
                gw, gb = torch.zeros(D, device=dev), (None if b is None else torch.zeros(1, device=dev))
                xa = x.clone().requires_grad_(True)
                wa = w.clone().requires_grad_(True)
                ba = None if b is None else b.clone().requires_grad_(True)
                loss_fn = torch.nn.BCELoss() if kind == "binary" else torch.nn.MSELoss()

                def fused():
                    s, pred, loss = ops.seq_task_fwd(x, None, w.view(-1), b, t, mode, act, lk)
                    return loss, ops.seq_task_bwd_(one, pred, t, s, None, L, w.view(-1), mode, act, lk, gw, gb)

                def chain():
                    xa.grad = wa.grad = None
                    if ba is not None:
                        ba.grad = None
                    s = xa.mean(1) if summary == "mean" else (xa[:, 0] if summary == "first" else xa[:, -1])
                    z = F.linear(s, wa, ba)
                    p = torch.sigmoid(z) if kind == "binary" else z
                    loss = loss_fn(p.squeeze(-1), t)
                    loss.backward()
                    return loss, xa.grad

                gw.zero_()
                (la, dxa), (lb, dxb) = fused(), chain()
                torch.cuda.synchronize()
                agree = dict(loss=float((la.view(()) - lb).abs()), dx=float((dxa - dxb).abs().max()),
                             d_w=float((gw - wa.grad.view(-1)).abs().max()))
                assert agree["loss"] < 1e-5 and agree["dx"] < 1e-6 and agree["d_w"] < 1e-5, agree
                for fn in (fused, chain):           # warm-up
                    _timed(fn, inner)
                tf, tc = [], []
                for _ in range(reps):               # alternating
                    tf.append(_timed(fused, inner))
                    tc.append(_timed(chain, inner))
                row = dict(B=B, L=L, D=D, task=kind, summary=summary, max_abs_diff=agree)
                row.update({"fused_" + k: v for k, v in _stats(tf, "us").items()})
                row.update({"chain_" + k: v for k, v in _stats(tc, "us").items()})
                row["faster_by_more_than_the_larger_spread"] = bool(row["chain_us"] - row["fused_us"] > max(row["fused_us_iqr"], row["chain_us_iqr"]))
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


def training_step(reps):
    """ms per training step of the configs[1]-shaped model, next-item task alone and with a binary `mean` task added"""
    import transformers4rec_amd as tr

    V, D, L = 100_000, 128, 20
    schema = tr.session_schema(V, L)
    runs, out = {}, {}
    for form in ("next_item", "next_item_plus_binary_mean"):
        torch.manual_seed(0)
        inputs = tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=L, masking="clm", aggregation="concat",
                                                        embedding_dims={"item_id": D})
        tasks = [tr.NextItemPredictionTask(weight_tying=True)]
        if form != "next_item":
            tasks.append(tr.BinaryClassificationTask("click", summary_type="mean"))
        model = tr.XLNetConfig.build(D, 4, 4, total_seq_length=L, dropout=0.3).to_torch_model(inputs, *tasks).to("cuda")
        dense, tables = tr.flatten_model(model)
        opt = tr.FusedAdam([dense, tables], lr=1e-3)
        batches = [{k: v.to("cuda") for k, v in tr.random_data_from_schema(schema, B, L, seed=100 + i).items()} for i in range(4)]
        g = torch.Generator().manual_seed(1)
        targets = {"click": torch.randint(0, 2, (B,), generator=g).float().to("cuda")}

        def step(i, model=model, opt=opt, batches=batches, targets=targets):
            opt.zero_grad()
            model(batches[i % 4], targets=targets, training=True)["loss"].backward()
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
        raise SystemExit("seq_task_bench: no GPU visible; a timing needs one")
    reps, inner = _arg("--reps", 200, int), _arg("--inner", 5, int)
    path = _arg("--out", os.path.join(ROOT, "profiles", "seq_task_ab.json"), str)
    assert reps >= 200, "each figure is the median over at least 200 samples"
    res = dict(device=torch.cuda.get_device_name(0), reps=reps, inner=inner,
               method="median over reps of device-event time per forward + backward pair, fused and chain alternating in one "
                      "process; spread = interquartile range", kernels=kernels_ab(reps, inner))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    if "--no-step" not in sys.argv:
        res["training_step_configs1_shape"] = training_step(max(40, reps // 5))
        print(json.dumps(res["training_step_configs1_shape"]), flush=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
