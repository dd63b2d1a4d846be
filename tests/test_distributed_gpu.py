"""The N > 1 training step on REAL kernels: two processes share the one GPU of the test box and exchange gradients
over gloo (RCCL refuses two ranks on one device; the collectives are the only thing swapped out).  bench.py's own
wiring -- setup_data_parallel (row-sparse sink on the tables, async table all-reduce hooked after the head's
backward), make_train_step, FusedAdam with 1/world folded in -- must (a) leave the replicas bit-identical after
several steps and (b) equal a single process that averages the two ranks' gradients itself."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

V, D, NL, NH, L, B, STEPS = 5000, 64, 2, 4, 20, 64, 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _build(device):
    import bench

    return bench.build(device, 0.0, v_items=V, d_model=D, n_layer=NL, n_head=NH, seq=L, lr=1e-2)


def _batches(tr, schema, rank, device):
    return [tr.random_data_from_schema(schema, B, L, seed=100 * rank + i, device=device) for i in range(STEPS)]


def _worker(rank, world, port, ret, mode="sparse"):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import bench

    tr, schema, model, dense, tables, opt = _build(dev)
    reducer, hook = bench.setup_data_parallel(tr, model, dense, tables, world, mode=mode)
    if mode == "sparse":
        assert hook is not None and reducer.sparse is not None
    else:           # "dense": every rank scatters its own lookups, ONE table all-reduce at the end -- no hook, nothing row-sparse
        assert hook is None and reducer.sparse is None
    model.input_features.masking.seed, model.transformer_block.transformer.seed = bench.rank_seeds(rank)
    model.train()
    batches = _batches(tr, schema, rank, dev)
    # step 0 by hand (the same calls make_train_step makes) to look at the EXCHANGED gradients before Adam eats them
    out = model(batches[0], training=True)
    out["loss"].backward()
    reducer.reduce_all()
    grads0 = torch.cat([f.grad for f in opt.flats]).cpu() * reducer.grad_scale
    opt.step(grad_scale=reducer.grad_scale)
    step = bench.make_train_step(model, batches, reducer, opt)
    losses = [float(out["loss"].detach())] + [float(step(i)["loss"].detach()) for i in range(1, STEPS)]
    torch.cuda.synchronize()
    flat = torch.cat([f.data for f in opt.flats]).cpu()
    both = [torch.zeros_like(flat) for _ in range(world)]
    dist.all_gather(both, flat)
    if rank == 0:
        ret.update(identical=torch.equal(both[0], both[1]), grads0=grads0, losses=losses,
                   bytes=reducer.sparse.bytes_exchanged if reducer.sparse is not None else 0)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["sparse", "dense"])
def test_two_rank_training_step_on_one_gpu(mode):
    """both forms of the table-gradient exchange (bench.py times them at N > 1 and keeps the faster: either may run)"""
    world = 2
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), ret, mode), nprocs=world, join=True)
    assert ret["identical"], "replicas drifted: the gradient exchange is not the same on both ranks"
    assert (ret["bytes"] > 0) == (mode == "sparse")
    # single-process expectation for step 0: both ranks' batches, gradients averaged.  (Parameters after Adam are
    # not compared across implementations: m / sqrt(v) turns a last-bit difference of a near-zero gradient into a
    # full-size update; the split-K atomics already differ in the last bits from run to run.)
    import bench

    dev = torch.device("cuda", 0)
    tr, schema, model, dense, tables, opt = _build(dev)
    model.train()
    masking, xl = model.input_features.masking, model.transformer_block.transformer
    for r in range(world):                          # replay rank r's mask stream
        masking.seed, xl.seed = bench.rank_seeds(r)
        masking._rng_offset = 0
        out = model(_batches(tr, schema, r, dev)[0], training=True)
        out["loss"].backward()                      # the two ranks' gradients accumulate in the flat buckets
    torch.cuda.synchronize()
    want = torch.cat([f.grad for f in opt.flats]).cpu() / world
    got = ret["grads0"]
    scale = float(want.abs().max())
    assert scale > 0 and float((got - want).abs().max()) < 1e-4 * scale, (float((got - want).abs().max()), scale)
    assert ret["losses"][-1] < ret["losses"][0] + 0.5


# ------------------------------------------------------------------------------------------ torch DDP over the functional path
def _ddp_worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import transformers4rec_amd as tr
    from transformers4rec_amd import functional as F

    torch.manual_seed(0)
    schema = tr.session_schema(V, L)
    inputs = tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=L, masking="mlm", embedding_dim_default=D)
    cfg = tr.XLNetConfig.build(D, NH, NL, total_seq_length=L, dropout=0.0)
    model = cfg.to_torch_model(inputs, tr.NextItemPredictionTask(weight_tying=True)).to(dev).train()
    model.input_features.masking.seed = 1234 + rank
    fm = F.FunctionalMLMModel(model)
    ddp = torch.nn.parallel.DistributedDataParallel(fm)          # torch's own wrapper: bucket hooks on AccumulateGrad
    ids = tr.random_data_from_schema(schema, B, L, seed=300 + rank, device=dev)["item_id"]
    # what DDP must produce: the average over the ranks of each rank's own gradients
    loss = fm(ids)["loss"]
    own = torch.autograd.grad(loss, list(fm.parameters()))
    flat = torch.cat([g.reshape(-1) for g in own]).cpu()
    both = [torch.zeros_like(flat) for _ in range(world)]
    dist.all_gather(both, flat)
    want = (both[0] + both[1]) / 2
    model.input_features.masking._rng_offset = 0                  # the same mask again
    out = ddp(ids)
    out["loss"].backward()
    torch.cuda.synchronize()
    got = torch.cat([p.grad.reshape(-1) for p in fm.parameters()]).cpu()
    if rank == 0:
        ret.update(err=float((got - want).abs().max()), scale=float(want.abs().max()), n=int(out["n_labels"]))
    dist.barrier()
    dist.destroy_process_group()


def test_torch_ddp_wraps_the_functional_model():
    """with every parameter gradient an output of a registered operator, torch DDP's bucket hooks see
    them -- DistributedDataParallel(FunctionalMLMModel(model)) averages the two ranks' gradients (the drop-in built on the
    flat-buffer backward has to refuse DDP and exchange gradients itself)"""
    world = 2
    ret = mp.Manager().dict()
    mp.spawn(_ddp_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    assert ret["n"] > 0 and ret["scale"] > 0
    assert ret["err"] < 1e-6 + 1e-5 * ret["scale"], dict(ret)


def _ddp_session_worker(rank, world, port, ret):
    """as _ddp_worker, for the MULTI-FEATURE model at dropout 0.3 through functional.FunctionalSessionModel (round 5)"""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import transformers4rec_amd as tr
    from transformers4rec_amd import functional as F
    from transformers4rec_amd.rng import get_rng_state, set_rng_state

    torch.manual_seed(0)
    schema = tr.session_schema(V, L, (("category", 50), ("brand", 9)), ("price", "age"))
    inputs = tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=L, masking="mlm", aggregation="concat", d_output=D,
                                                    continuous_soft_embeddings=True, embedding_dims={"item_id": D},
                                                    embedding_dim_default=16)
    cfg = tr.XLNetConfig.build(D, NH, NL, total_seq_length=L, dropout=0.3)
    model = cfg.to_torch_model(inputs, tr.NextItemPredictionTask(weight_tying=True)).to(dev).train()
    model.input_features.masking.seed, model.transformer_block.transformer.seed = 1234 + rank, 77 + rank
    fm = F.FunctionalSessionModel(model)
    ddp = torch.nn.parallel.DistributedDataParallel(fm)
    batch = tr.random_data_from_schema(schema, B, L, seed=300 + rank, device=dev)
    state = get_rng_state(model)
    loss = fm(dict(batch))["loss"]
    own = torch.autograd.grad(loss, list(fm.parameters()))
    flat = torch.cat([g.reshape(-1) for g in own]).cpu()
    both = [torch.zeros_like(flat) for _ in range(world)]
    dist.all_gather(both, flat)
    want = (both[0] + both[1]) / 2
    set_rng_state(model, state)                                    # the same MLM and dropout masks again
    out = ddp(dict(batch))
    out["loss"].backward()
    torch.cuda.synchronize()
    got = torch.cat([p.grad.reshape(-1) for p in fm.parameters()]).cpu()
    if rank == 0:
        ret.update(err=float((got - want).abs().max()), scale=float(want.abs().max()), n=int(out["n_labels"]),
                   n_params=len(list(fm.parameters())))
    dist.barrier()
    dist.destroy_process_group()


def test_torch_ddp_wraps_the_multi_feature_functional_model():
    """torch's own DistributedDataParallel over the registered-operator form of a configs[2]-shaped model
    (item + two categoricals + two SoftEmbedding features, concat, projection) at dropout 0.3: the bucket hooks see every
    gradient -- tables, soft embeddings, projection, mask vector, layers -- and average them over the two ranks"""
    world = 2
    ret = mp.Manager().dict()
    mp.spawn(_ddp_session_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    assert ret["n"] > 0 and ret["scale"] > 0 and ret["n_params"] >= 3 + 10 + 2 + 1 + 15 * NL
    assert ret["err"] < 1e-6 + 1e-5 * ret["scale"], dict(ret)


def test_bench_main_two_ranks():
    """`bench.py --gpus 2` END TO END on real kernels -- the driver's N > 1 command with the collectives over gloo and both
    ranks on the box's one GPU (T4R_BENCH_BACKEND / T4R_BENCH_SHARE_GPU): warm-up, the timed pick of the table-gradient
    exchange, pre-heat with roll-back, the timed region, the per-rank roofline probes, the comm report and the data-parallel
    Recall@20 probe.  Round 4: this run found a name of the comm report shadowed by a probe -- a crash on every N > 1 run that
    no N = 1 run and no CPU stub run reaches."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, T4R_BENCH_BACKEND="gloo", T4R_BENCH_SHARE_GPU="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), "bench.py", "--gpus", "2", "--steps", "6", "--warmup", "2", "--preheat-seconds", "0.5", "--full"]
    run = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    line = json.loads(run.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and line["steps"] == 6 and line["scaling"] == "weak"
    assert line["config"]["world_size"] == 2 and line["config"]["collective_backend"] == "gloo"
    assert line["config"]["table_exchange"] in ("sparse", "dense")
    both = line["comm"]["table_exchange_ms_per_step"]
    assert set(both) == {"sparse", "dense"} and both[line["config"]["table_exchange"]] == min(both.values())
    assert line["comm"]["dense_bucket_bytes"] > 0 and line["value"] > 0
    assert "cpu_baseline" not in line                      # rank 0 at N = 1 only
    assert line["roofline"]["bound"] in ("hbm", "mfma") and 0 < line["roofline"]["frac"] < 1
    assert line["recall_at_20"]["hip_bench_config_dp"]["eval_sessions"] > 0


# ------------------------------------------------------------------------------------------------------------------
# Round 6: the MODULE path itself under torch DDP.  masking.GradCarrier routes the parameter gradients
# of the hot-path modules through autograd (same kernels, same numbers), so torch.nn.parallel.DistributedDataParallel --
# what HF Trainer wraps the reference's model in (transformers4rec/torch/trainer.py:131-161) -- can wrap the drop-in model.
def _multi_model(tr, dev, rank, dropin_convert):
    import types

    torch.manual_seed(0)
    schema = tr.session_schema(V, L, (("category", 50), ("brand", 9)), ("price", "age"))
    inputs = tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=L, masking="mlm", aggregation="concat", d_output=D,
                                                    continuous_soft_embeddings=True, embedding_dims={"item_id": D},
                                                    embedding_dim_default=16)
    cfg = tr.XLNetConfig.build(D, NH, NL, total_seq_length=L, dropout=0.3)
    model = cfg.to_torch_model(inputs, tr.NextItemPredictionTask(weight_tying=True)).to(dev).train()
    if dropin_convert:
        from transformers4rec_amd import dropin

        ns = types.SimpleNamespace(TabularSequenceFeatures=tr.TabularSequenceFeatures, TransformerBlock=tr.TransformerBlock,
                                   NextItemPredictionTask=tr.NextItemPredictionTask)
        dropin.convert_model(model, ns)
        masking, xl = model.input_features.hip_shadow().masking, model.transformer_block.hip_shadow().transformer
    else:
        masking, xl = model.input_features.masking, model.transformer_block.transformer
    masking.seed, xl.seed = 1234 + rank, 77 + rank
    return schema, model, masking, xl


def _reset(masking, xl):
    masking._rng_offset, xl._drop_offset = 0, 0


@pytest.mark.parametrize("dropin_convert", [False, True], ids=["mirror", "dropin"])
def test_autograd_visible_gradients_equal_the_fast_path(dropin_convert):
    """enable_autograd_gradients: every parameter gradient arrives through autograd (hooks fire, torch.autograd.grad works) and
    equals, bit for bit, what the fast path writes into .grad"""
    import transformers4rec_amd as tr

    dev = torch.device("cuda", 0)
    schema, model, masking, xl = _multi_model(tr, dev, 0, dropin_convert)
    batch = tr.random_data_from_schema(schema, B, L, seed=300, device=dev)
    _reset(masking, xl)
    model(dict(batch), training=True)["loss"].backward()
    torch.cuda.synchronize()
    fast = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    for p in model.parameters():
        p.grad = None
    if dropin_convert:
        from transformers4rec_amd import dropin

        dropin.enable_ddp(model)
    else:
        tr.enable_autograd_gradients(model)
    fired = []
    hooks = [p.register_hook(lambda g, n=n: fired.append(n)) for n, p in model.named_parameters()]
    _reset(masking, xl)
    model(dict(batch), training=True)["loss"].backward()
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    assert len(fast) > 30 and set(fast) <= set(fired)
    for n, p in model.named_parameters():
        if n in fast:       # same kernels, same inputs.  At this small size (V 5000, 64 sessions) the head and a few reductions run the
            # general split-K GEMM with fp32 atomics: two runs of the FAST path differ by as much (test_training_mode_dropout_
            # end_to_end); the bit-reproducible forms start at the sizes of BASELINE configs[1]
            torch.testing.assert_close(p.grad, fast[n], rtol=1e-4, atol=2e-5 * float(fast[n].abs().max()) + 1e-9,
                                       msg=lambda m, n=n: f"{n}: {m}")
        else:       # parameters the path never touches (HF's seg_embed, r_s_bias, ...): a zero gradient, not a missing one
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
        assert "_t4r_carrier" not in p.__dict__
    # torch.autograd.grad sees them too
    _reset(masking, xl)
    loss = model(dict(batch), training=True)["loss"]
    names = [n for n in fast]
    params = dict(model.named_parameters())
    got = torch.autograd.grad(loss, [params[n] for n in names])
    for n, g in zip(names, got):
        torch.testing.assert_close(g, fast[n], rtol=1e-4, atol=2e-5 * float(fast[n].abs().max()) + 1e-9, msg=lambda m, n=n: f"{n}: {m}")
    # evaluation and a second training step still work (carriers of a forward without backward are dropped)
    model.eval()
    with torch.no_grad():
        model(dict(batch), testing=True)
    model.train()
    model(dict(batch), training=True)
    _reset(masking, xl)
    for p in model.parameters():
        p.grad = None
    model(dict(batch), training=True)["loss"].backward()
    torch.testing.assert_close(params[names[0]].grad, fast[names[0]], rtol=1e-4, atol=2e-5 * float(fast[names[0]].abs().max()) + 1e-9)


def _ddp_dropin_worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import transformers4rec_amd as tr
    from transformers4rec_amd import dropin

    schema, model, masking, xl = _multi_model(tr, dev, rank, True)
    batch = tr.random_data_from_schema(schema, B, L, seed=300 + rank, device=dev)
    # the guard still refuses the fast path on > 1 ranks ...
    try:
        model(dict(batch), training=True)
        refused = False
    except RuntimeError as e:
        refused = "enable_ddp" in str(e)
    # ... each rank's own gradients on the fast path, acknowledged (what GradReducer / sync_gradients would average)
    dropin.enable_data_parallel(model)
    _reset(masking, xl)
    model(dict(batch), training=True)["loss"].backward()
    torch.cuda.synchronize()
    names = [n for n, p in model.named_parameters() if p.grad is not None]
    flat = torch.cat([p.grad.reshape(-1) for n, p in model.named_parameters() if n in names]).cpu()
    both = [torch.zeros_like(flat) for _ in range(world)]
    dist.all_gather(both, flat)
    want = (both[0] + both[1]) / 2
    for p in model.parameters():
        p.grad = None
    # ... and torch DDP over the same model in the autograd-visible mode
    dropin.enable_ddp(model)
    ddp = torch.nn.parallel.DistributedDataParallel(model)
    _reset(masking, xl)
    out = ddp(dict(batch), training=True)
    out["loss"].backward()
    torch.cuda.synchronize()
    got = torch.cat([p.grad.reshape(-1) for n, p in model.named_parameters() if n in names]).cpu()
    # three more DDP steps with a torch optimizer: the replicas stay identical
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    for i in range(3):
        opt.zero_grad()
        b = tr.random_data_from_schema(schema, B, L, seed=900 + 10 * i + rank, device=dev)
        ddp(dict(b), training=True)["loss"].backward()
        opt.step()
    torch.cuda.synchronize()
    w = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu()
    ws = [torch.zeros_like(w) for _ in range(world)]
    dist.all_gather(ws, w)
    if rank == 0:
        ret.update(err=float((got - want).abs().max()), scale=float(want.abs().max()), n=len(names), refused=refused,
                   replicas_equal=bool(torch.equal(ws[0], ws[1])))
    dist.barrier()
    dist.destroy_process_group()


def test_torch_ddp_wraps_the_dropin_model():
    """torch DistributedDataParallel over the drop-in model itself (dropin.enable_ddp): gradients == the average of the two ranks'
    fast-path gradients (what distributed.GradReducer / dropin.sync_gradients exchange), replicas identical after Adam steps"""
    world = 2
    ret = mp.Manager().dict()
    mp.spawn(_ddp_dropin_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    assert ret["refused"] and ret["n"] > 30 and ret["scale"] > 0
    assert ret["err"] < 1e-7 + 1e-6 * ret["scale"], dict(ret)
    assert ret["replicas_equal"]
