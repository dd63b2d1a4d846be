"""Sampling heads on the GPU (include/t4r_hip_sampling.h): Gumbel noise over materialised scores (csrc/item_sample.hip), the two
fused top-k heads as samplers (ops.item_sample: the noisy collect epilogues of csrc/gemm_kernel.h and csrc/item_topk_h16.hip),
NextItemPredictionTask.sample_items, LazyPredictions.sample and the replacement-token masking built on them.

The contract is the top-k heads': the fused result equals the MATERIALISED composition
    topk(gumbel_add_(item_scores(x, W, alpha).clone(), seed, ctr_hi, row0), k)
bit for bit (values, ids, order), because a perturbed score is a pure function of (seed, ctr_hi, row, item).  The noise itself is
checked against its numpy restatement (tests/gumbel_restatement.py)."""
import ctypes

import numpy as np
import pytest
import torch

import gumbel_restatement as gr
import test_abi_redzone_gpu as rz

DEV = "cuda"
gpu = pytest.mark.gpu
SEED = 1234


def _strided(t, extra):
    n, d = t.shape
    buf = torch.empty((n, d + extra), device=t.device, dtype=t.dtype)
    buf[:, :d] = t
    return buf[:, :d]


def _inputs(N, V, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((N, D), generator=g), torch.randn((V, D), generator=g)


def _table(ops, Wd, table):
    return Wd if table == "fp32" else ops.pack_item_table(Wd, table)


def _composition(ops, xd, Wt, k, alpha, seed, ctr_hi, row0=0):
    with ops.precision("fp32"):                       # the fp32 table's materialised scores in form 0; an image ignores the mode
        s = ops.item_scores(xd, Wt, alpha).clone()
    return ops.topk(ops.gumbel_add_(s, seed, ctr_hi, row0), k)


# ------------------------------------------------------------------------------------------------ 1. the noise
@gpu
@pytest.mark.parametrize("n,V,ld,row0,stride", [(7, 1001, 1004, 0, 1), (5, 333, 336, 6, 3)])
def test_gumbel_add_against_the_restatement(n, V, ld, row0, stride):
    from transformers4rec_amd import _lib

    g = torch.Generator().manual_seed(n + V)
    s = 3.0 * torch.randn((n, V), generator=g)
    buf = torch.full((n, ld), 7.25, device=DEV)
    buf[:, :V] = s.to(DEV)
    ctr = gr.ctr_hi_of(5)
    _lib.call("t4r_gumbel_add_f32", torch.cuda.current_stream().cuda_stream, buf.data_ptr(), n, V, ld, row0, stride, SEED, ctr)
    got = buf.cpu()
    gn = gr.gumbel(SEED, ctr, row0 + np.arange(n), np.arange(V) * stride)
    want = (s.double().numpy() + gn).astype(np.float32)
    bound = 2.0 ** -18 * np.maximum(1.0, np.abs(s.double().numpy()) + np.abs(gn))
    err = np.abs(got[:, :V].double().numpy() - want.astype(np.float64))
    print(f"[gumbel_add] {n} x {V} row0 {row0} stride {stride}: largest error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    assert bool((got[:, V:] == 7.25).all())                                   # pad columns unchanged


@gpu
@pytest.mark.parametrize("N,V", [(33, 5003), (3, 70001)])
def test_gumbel_argmax_equals_add_then_topk(N, V):
    from transformers4rec_amd import ops

    g = torch.Generator().manual_seed(N + V)
    s = _strided((2.0 * torch.randn((N, V), generator=g)).to(DEV), 5)
    ctr = gr.ctr_hi_of(2)
    keep = s.clone()
    v, i = ops.gumbel_argmax(s, SEED, ctr, row0=3)
    assert torch.equal(s, keep)                                               # the scores are read, not written
    rv, ri = ops.topk(ops.gumbel_add_(s.clone(), SEED, ctr, row0=3), 1)
    assert v.shape == (N,) and i.dtype == torch.int64
    assert torch.equal(i, ri[:, 0]) and torch.equal(v, rv[:, 0])
    assert int((i != s.argmax(1)).sum()) > 0                                  # the noise decides somewhere


@gpu
def test_gumbel_argmax_ties_go_to_the_lower_index():
    from transformers4rec_amd import ops

    s = torch.randn((6, 4000), generator=torch.Generator().manual_seed(1)).to(DEV)
    s[:, 1234] = 2.0 ** 30                     # half an ulp at 2^30 is 64 > 16.64: the noise is absorbed, the two columns tie
    s[:, 77] = 2.0 ** 30
    v, i = ops.gumbel_argmax(s, SEED, gr.ctr_hi_of(9))
    assert i.tolist() == [77] * 6 and bool((v == 2.0 ** 30).all())
    rv, ri = ops.topk(ops.gumbel_add_(s.clone(), SEED, gr.ctr_hi_of(9)), 1)
    assert torch.equal(i, ri[:, 0]) and torch.equal(v, rv[:, 0])


# ------------------------------------------------------------------------------------------------ 3. fused == materialised
SHAPES = [(1, 7, 8, 7, 1.0), (37, 5003, 40, 1, 1.0), (130, 5003, 40, 20, 0.5), (33, 65537, 100, 1, 1.0), (70, 20011, 32, 256, 1.0)]


@gpu
@pytest.mark.parametrize("table", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("N,V,D,k,alpha", SHAPES)
def test_item_sample_equals_the_materialised_composition(N, V, D, k, alpha, table):
    from transformers4rec_amd import ops

    x, W = _inputs(N, V, D, N + V + k)
    xd = _strided(x.to(DEV), 1 if D % 2 == 0 else 2)
    Wt = _table(ops, _strided(W.to(DEV), 3 if D % 2 == 0 else 2), table)
    ctr = gr.ctr_hi_of(N)
    calls = ops.item_topk_stats()["calls"]
    vals, ids = ops.item_sample(xd, Wt, k, SEED, ctr, alpha=alpha)
    st = ops.item_topk_stats()
    rv, ri = _composition(ops, xd, Wt, k, alpha, SEED, ctr)
    print(f"[item_sample {table}] N {N} V {V} D {D} k {k}: sample {st['sample_rows']} cap {st['list_capacity']} "
          f"fallback rows {st['fallback_rows']}")
    assert vals.shape == (N, k) and ids.shape == (N, k) and ids.dtype == torch.int64 and vals.dtype == torch.float32
    assert torch.equal(ids, ri)
    assert torch.equal(vals, rv)
    assert st["calls"] == calls + 1 and st["dtype"] == table
    assert st["fallback_rows"] == 0                                           # Gaussian inputs
    if V == 5003:
        assert st["sample_rows"] == 1024                                      # stride 4 and a pad column in the sample buffer
    if k < V:
        assert not torch.equal(ids, ops.item_topk(xd, Wt, k, alpha=alpha)[1])  # a sample, not the top-k


# ------------------------------------------------------------------------------------------------ 4. overflow
@gpu
@pytest.mark.parametrize("table", ["fp32", "bf16"])
def test_overflow_rows_take_the_materialised_path(table):
    from transformers4rec_amd import ops

    N, V, D, k = 12, 5000, 32, 10
    x, W = _inputs(N, V, D, 13)
    best = 2.0 * W[17]                      # |best|^2 ~ 128 against |best . w| <~ 45 for the other rows of W
    big = [0, 1, 2, 5, 9, 10]
    x[big] = best * 2.0 ** 25
    sel = torch.randperm(V, generator=torch.Generator().manual_seed(7))[:3000]
    W[sel] = best
    xd = x.to(DEV)
    Wt = _table(ops, W.to(DEV), table)
    with ops.precision("fp32"):
        s = ops.item_scores(xd, Wt).cpu()
    copies = torch.zeros(V, dtype=torch.bool)
    copies[sel] = True
    # the case is what it says: the copies tie far above 2^30 (half an ulp >= 64 > the noise) and far above every other item
    assert float(s[big][:, copies].min()) > 2.0 ** 30 and float(s[big][:, copies].min() - s[big][:, ~copies].max()) > 2.0 ** 30
    assert bool((s[big][:, copies] == s[big][:, copies][:, :1]).all())
    ctr = gr.ctr_hi_of(4)
    v, i = ops.item_sample(xd, Wt, k, SEED, ctr)
    st = ops.item_topk_stats()
    rv, ri = _composition(ops, xd, Wt, k, 1.0, SEED, ctr)
    print(f"[item_sample overflow {table}] fallback rows {st['fallback_rows']} of {N} (sample {st['sample_rows']}, cap {st['list_capacity']})")
    assert st["fallback_rows"] == 6
    assert torch.equal(i, ri) and torch.equal(v, rv)
    lowest = sorted(sel.tolist())[:k]
    for r in big:
        assert i[r].tolist() == lowest                                        # the noise is absorbed: ties, lowest ids first
    v2, i2 = ops.item_sample(xd, Wt, k, SEED, ctr)
    assert torch.equal(i, i2) and torch.equal(v, v2)


# ------------------------------------------------------------------------------------------------ 5. keys
@gpu
@pytest.mark.parametrize("table", ["fp32", "fp16"])
def test_keys_replay_and_rows_are_addressed_by_row0(table):
    from transformers4rec_amd import ops

    N, V, D, k = 40, 5003, 40, 5
    x, W = _inputs(N, V, D, 3)
    xd = x.to(DEV)
    Wt = _table(ops, W.to(DEV), table)
    v, i = ops.item_sample(xd, Wt, k, SEED, gr.ctr_hi_of(1))
    v2, i2 = ops.item_sample(xd, Wt, k, SEED, gr.ctr_hi_of(1))
    assert torch.equal(v, v2) and torch.equal(i, i2)
    _, j = ops.item_sample(xd, Wt, k, SEED, gr.ctr_hi_of(2))
    assert int((i[:, 0] != j[:, 0]).sum()) > N // 2                           # another offset: other draws in most rows
    _, j = ops.item_sample(xd, Wt, k, SEED + 1, gr.ctr_hi_of(1))
    assert int((i[:, 0] != j[:, 0]).sum()) > N // 2                           # another key
    pv, pi = ops.item_sample(xd[8:20], Wt, k, SEED, gr.ctr_hi_of(1), row0=8)
    assert torch.equal(pv, v[8:20]) and torch.equal(pi, i[8:20])


# ------------------------------------------------------------------------------------------------ 6. frequencies
@gpu
@pytest.mark.parametrize("table", ["fp32", "fp16"])
def test_frequencies_through_the_fused_head(table):
    from transformers4rec_amd import ops

    logits = gr.freq_logits()
    W = torch.from_numpy(logits).float().view(61, 1).to(DEV)
    Wt = _table(ops, W, table)
    x = torch.ones((40000, 1), device=DEV)
    _, ids = ops.item_sample(x, Wt, 1, 99, gr.ctr_hi_of(1))
    chi2, min_expected = gr.chi2_of_argmax(ids.cpu().numpy(), Wt.double().cpu().numpy()[:, 0])
    print(f"[item_sample frequencies {table}] chi2 {chi2:.1f} (bound {gr.CHI2_60_Q999}), smallest expected count {min_expected:.1f}")
    assert ops.item_topk_stats()["fallback_rows"] == 0
    assert chi2 < gr.CHI2_60_Q999


# ------------------------------------------------------------------------------------------------ 7. the task
def _tiny_model(masking, task_block=False, head_mode="auto", V=3001, L=20, D=64):
    import transformers4rec_amd as tr

    schema = tr.session_schema(V - 1, L)
    torch.manual_seed(0)
    kw = dict(d_output=D, embedding_dims={"item_id": 24}, aggregation="concat") if task_block else dict(embedding_dim_default=D)
    inputs = tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=L, masking=masking, **kw)
    cfg = tr.XLNetConfig.build(D, 4, 1, total_seq_length=L, dropout=0.0)
    model = cfg.to_torch_model(inputs, tr.NextItemPredictionTask(weight_tying=True, head_mode=head_mode, softmax_temperature=2.0))
    return model.to(DEV).eval(), schema


def _hidden(model, ids, **kw):
    cap = {}
    h = model.transformer_block.register_forward_hook(lambda m, i, o: cap.__setitem__("hid", o))
    with torch.no_grad():
        out = model({"item_id": ids}, **kw)
    h.remove()
    hid = cap["hid"]
    return out, (hid[0] if isinstance(hid, (tuple, list)) else hid)


@gpu
@pytest.mark.parametrize("masking,task_block", [("mlm", False), ("clm", False), ("mlm", True)])
def test_task_sample_items(masking, task_block):
    import transformers4rec_amd as tr
    from transformers4rec_amd import ops

    B, L, k = 24, 20, 4
    model, schema = _tiny_model(masking, task_block)
    task = model.prediction_task
    assert (task.task_block is not None) == task_block
    ids = tr.random_data_from_schema(schema, B, L, seed=4)["item_id"].to(DEV)
    scores, hid = _hidden(model, ids)
    task.sample_seed = 4321
    assert task._sample_offset == 0
    state = tr.get_rng_state(model)
    v, i = task.sample_items(hid, k=k)
    assert task._sample_offset == 1 and v.shape == (B, k) and i.shape == (B, k)
    xr, inv_t = task._inference_rows(hid.float())
    assert inv_t == 0.5
    W = task.pre.module.output_weights.detach()
    rv, ri = ops.item_sample(xr, W, k, 4321, gr.ctr_hi_of(1), inv_t)
    assert torch.equal(v, rv) and torch.equal(i, ri)
    with ops.precision("fp32"):                        # the rows are the inference forward's: its scores, perturbed, give the draw
        s32 = ops.item_scores(xr, W, inv_t)
    cv, ci = ops.topk(ops.gumbel_add_(s32.clone(), 4321, gr.ctr_hi_of(1)), k)
    assert torch.equal(v, cv) and torch.equal(i, ci)
    v2, i2 = task.sample_items(hid, k=k)
    assert task._sample_offset == 2 and not torch.equal(i, i2)                # the stream advances
    tr.set_rng_state(model, state)
    assert task._sample_offset == 0
    v3, i3 = task.sample_items(hid, k=k)
    assert torch.equal(v3, v) and torch.equal(i3, i)                          # ... and replays
    # with a serving image: the 16-bit head over the image
    task.prepare_serving("fp16")
    h16 = ops.item_topk_stats()["calls_h16"]
    v4, i4 = task.sample_items(hid, k=k)
    assert ops.item_topk_stats()["calls_h16"] == h16 + 1 and ops.item_topk_stats()["dtype"] == "fp16"
    rv, ri = ops.item_sample(xr, ops.pack_item_table(W, "fp16"), k, 4321, gr.ctr_hi_of(2), inv_t)
    assert torch.equal(v4, rv) and torch.equal(i4, ri)
    task.drop_serving_image()
    # forward is what it was: the inference scores of the same hidden states
    with torch.no_grad():
        again = task(hid)
    assert torch.equal(again, scores)


@gpu
def test_operators_equal_the_ctypes_calls():
    from transformers4rec_amd import ops, torch_ops  # noqa: F401

    x, W = _inputs(50, 3001, 64, 8)
    xd, Wd = x.to(DEV), W.to(DEV)
    ctr = gr.ctr_hi_of(3)
    v, i = torch.ops.t4r_hip.item_sample(xd, Wd, 0.5, 10, SEED, ctr, 2)
    rv, ri = ops.item_sample(xd, Wd, 10, SEED, ctr, alpha=0.5, row0=2)
    assert torch.equal(v, rv) and torch.equal(i, ri)
    s = ops.item_scores(xd, Wd)
    v, i = torch.ops.t4r_hip.gumbel_argmax(s, SEED, ctr, 0)
    rv, ri = ops.gumbel_argmax(s, SEED, ctr)
    assert torch.equal(v, rv) and torch.equal(i, ri)
    torch.library.opcheck(torch.ops.t4r_hip.item_sample.default, (xd, Wd, 0.5, 10, SEED, ctr, 2),
                          test_utils=("test_schema", "test_faketensor"))


# ------------------------------------------------------------------------------------------------ 8. RTD end to end
@gpu
@pytest.mark.parametrize("from_batch", [False, True])
def test_rtd_end_to_end_in_both_head_modes(from_batch):
    import transformers4rec_amd as tr
    from transformers4rec_amd import masking as M, ops
    from transformers4rec_amd.prediction_task import LazyPredictions

    B, L = 16, 20
    triples, draws = {}, {}
    for mode in ("materialize", "fused"):
        model, schema = _tiny_model("rtd", head_mode=mode)
        m = model.input_features.masking
        assert type(m) is M.ReplacementLanguageModeling
        m.sample_from_batch = from_batch
        m.seed = 777
        ids = tr.random_data_from_schema(schema, B, L, seed=5)["item_id"].to(DEV)
        with ops.precision("fp32"):
            with torch.no_grad():
                out = model({"item_id": ids}, training=True)
            logits = out["predictions"]
            assert isinstance(logits, LazyPredictions) == (mode == "fused")
            target_flat = m.masked_targets.flatten()
            if from_batch:          # logits over the label rows of the batch (reference :799-802): [N_m, N_m]
                full = logits.materialize() if mode == "fused" else logits
                logits = full[:, out["labels"]].contiguous()
            assert m._sample_offset == 0
            triples[mode] = m.get_fake_tokens(ids, target_flat, logits)
            assert m._sample_offset == 1
            if mode == "fused" and not from_batch:
                assert not logits.is_materialized                             # the draw did not form the [N_m, V] logits
            m._sample_offset = 0
            draws[mode] = m.sample_from_softmax(logits)
        cin, dlab, upd = triples[mode]
        want = gr.fake_tokens_formula(ids, target_flat, draws[mode], 0, from_batch)
        assert torch.equal(cin, want[0]) and torch.equal(dlab, want[1])
        assert torch.equal(upd, want[2]) if from_batch else upd == []
        labelled = (target_flat != 0).view(B, L)
        assert int(labelled.sum()) == out["labels"].numel() > 0
        assert torch.equal(cin[~labelled], ids[~labelled]) and not bool(dlab[~labelled].any())
        assert torch.equal(dlab, cin != ids)
        assert bool(dlab.any())
    for a, b in zip(triples["materialize"], triples["fused"]):
        assert (torch.equal(a, b) if torch.is_tensor(a) else a == b)
    assert torch.equal(draws["materialize"], draws["fused"])


# ------------------------------------------------------------------------------------------------ 9. red zones and poison
def _noise_ref(key, n, cols, row0, stride, ctr):
    return rz.memo((key, "g"), lambda: torch.from_numpy(gr.gumbel(SEED, ctr, row0 + np.arange(n), np.arange(cols) * stride)))


def _rz_gumbel(n, V, ld, row0, stride):
    """t4r_gumbel_add_f32 in place on a pitched window; t4r_gumbel_argmax_f32 of the untouched scores against t4r_topk(1) of the
    perturbed ones (stride 1 only: argmax has no item stride)"""
    def fn(a, key):
        ctr = gr.ctr_hi_of(6)
        s = rz.dy(rz.gen(n + V), n, V)
        gn = _noise_ref(key, n, V, row0, stride, ctr)
        S = a.new("scores", "inout", rz.F32, (n, ld), 0, V).set(s)
        outs = []
        if stride == 1:
            S0 = a.new("scores_ro", "in", rz.F32, (n, ld), 0, V).set(s)
            AV, AI = a.new("argmax_val", "out", rz.F32, n), a.new("argmax_idx", "out", rz.I64, n)
            TV, TI = a.new("topk_val", "out", rz.F32, (n, 1)), a.new("topk_idx", "out", rz.I64, (n, 1))
            rz.call(a, "t4r_gumbel_argmax_f32", rz.stream(), S0.ptr, n, V, ld, row0, SEED, ctr, AV.ptr, AI.ptr)
        rz.call(a, "t4r_gumbel_add_f32", rz.stream(), S.ptr, n, V, ld, row0, stride, SEED, ctr)
        t = "test_sampling_gpu.py::test_gumbel_add_against_the_restatement (2^-18 max(1, |s| + |g|); |s| <= 3/8, |g| <= 16.64)"
        outs.append(rz.Out(S, s.double() + gn, dict(rtol=0, atol=2.0 ** -18 * 17.1), t))
        if stride == 1:
            rz.call(a, "t4r_topk", rz.stream(), S.ptr, n, V, ld, 1, TV.ptr, TI.ptr)
            torch.cuda.synchronize()
            assert torch.equal(AV.win, TV.win[:, 0]) and torch.equal(AI.win, TI.win[:, 0]), "argmax != topk(add, 1)"
            outs += [rz.Out(AV), rz.Out(AI)]
        return outs
    return fn


def _rz_item_sample(n, V, D, k, table, row0):
    """t4r_item_sample_f32 / _h16 with exact workspaces against the composition built in the same arena"""
    def fn(a, key):
        from transformers4rec_amd import ops

        lib = rz._lib().load()
        ctr = gr.ctr_hi_of(7)
        g = rz.gen(n * 3 + V + D)
        x, W = rz.dy(g, n, D), rz.dy(g, V, D)
        alpha = 0.5
        gn = _noise_ref(key, n, V, row0, 1, ctr)
        ref = rz.memo((key, "ref"), lambda: torch.sort(alpha * x.double() @ W.double().t() + gn, dim=1, descending=True).values[:, :k])
        ldx, ldw, ldc = D + 4, D + 4, (V + 3) // 4 * 4 + 4
        X, Wb = a.new("X", "in", rz.F32, (n, ldx), 0, D).set(x), a.new("W", "in", rz.F32, (V, ldw), 0, D).set(W)
        OV, OI = a.new("out_val", "out", rz.F32, (n, k)), a.new("out_idx", "out", rz.I64, (n, k))
        C = a.new("C", "out", rz.F32, (n, ldc), 0, V)
        TV, TI = a.new("topk_val", "out", rz.F32, (n, k)), a.new("topk_idx", "out", rz.I64, (n, k))
        st = (ctypes.c_long * 8)()
        if table == "fp32":
            nb = lib.t4r_item_sample_ws_bytes(n, V, D, k)
            WS = a.ws("workspace", nb)
            rz.call(a, "t4r_item_sample_f32", rz.stream(), n, V, D, alpha, X.ptr, ldx, Wb.ptr, ldw, k, OV.ptr, OI.ptr, WS.ptr, nb,
                    ctypes.cast(st, ctypes.c_void_p), row0, SEED, ctr)
            with ops.precision("fp32"):
                ops.gemm(X.win, Wb.win, False, True, alpha=alpha, out=C.win)
        else:
            td, code = (torch.float16, 3) if table == "fp16" else (torch.bfloat16, 2)
            ild = lib.t4r_item_table_image_ld(D)
            ldp = ild + 8
            IM = a.new("image", "out", td, (V, ldp), 0, D).allow(D, ldp)
            WS1 = a.ws("scores_ws", n * ild * 2)
            nb = lib.t4r_item_sample_h16_ws_bytes(n, V, D, k)
            WS = a.ws("workspace", nb)
            rz.call(a, "t4r_item_table_pack_h16", rz.stream(), Wb.ptr, ldw, V, D, code, IM.ptr, ldp)
            rz.call(a, "t4r_item_sample_h16", rz.stream(), n, V, D, alpha, X.ptr, ldx, IM.ptr, ldp, code, k, OV.ptr, OI.ptr, WS.ptr,
                    nb, ctypes.cast(st, ctypes.c_void_p), row0, SEED, ctr)
            rz.call(a, "t4r_item_scores_h16", rz.stream(), n, V, D, alpha, X.ptr, ldx, IM.ptr, ldp, code, C.ptr, ldc, WS1.ptr,
                    n * ild * 2)
        rz.call(a, "t4r_gumbel_add_f32", rz.stream(), C.ptr, n, V, ldc, row0, 1, SEED, ctr)
        rz.call(a, "t4r_topk", rz.stream(), C.ptr, n, V, ldc, k, TV.ptr, TI.ptr)
        torch.cuda.synchronize()
        assert torch.equal(OV.win, TV.win) and torch.equal(OI.win, TI.win), "item_sample != topk(gumbel_add(scores), k)"
        # exact inputs (multiples of 1/8, |score| <= D 9/128): the sorted perturbed scores against fp64
        t = "test_sampling_gpu.py::test_gumbel_add_against_the_restatement (2^-18 max(1, |s| + |g|))"
        return [rz.Out(OV, ref, dict(rtol=0, atol=2.0 ** -18 * (D * 9 / 128 + 17)), t), rz.Out(OI)]
    return fn


_ADD, _ARG = ["t4r_gumbel_add_f32"], ["t4r_gumbel_add_f32", "t4r_gumbel_argmax_f32"]
REDZONE_CASES = [
    rz.Case("sampling", "gumbel_add-7-1001-row6-stride3", _ADD, _rz_gumbel(7, 1001, 1004, 6, 3)),
    rz.Case("sampling", "gumbel_argmax-33-1000-row2", _ARG, _rz_gumbel(33, 1000, 1003, 2, 1)),
    rz.Case("sampling", "item_sample_f32-33-129-20-k20", ["t4r_item_sample_f32", "t4r_gumbel_add_f32"],
            _rz_item_sample(33, 129, 20, 20, "fp32", 5)),
    rz.Case("sampling", "item_sample_f32-1-1000-1-k1", ["t4r_item_sample_f32", "t4r_gumbel_add_f32"],
            _rz_item_sample(1, 1000, 1, 1, "fp32", 0)),
    rz.Case("sampling", "item_sample_h16-fp16-33-1000-512-k256", ["t4r_item_sample_h16", "t4r_gumbel_add_f32"],
            _rz_item_sample(33, 1000, 512, 256, "fp16", 3)),
    rz.Case("sampling", "item_sample_h16-bf16-1-7-1-k7", ["t4r_item_sample_h16", "t4r_gumbel_add_f32"],
            _rz_item_sample(1, 7, 1, 7, "bf16", 0)),
]
_RZ_BY_ID = {c.id: c for c in REDZONE_CASES}


@gpu
@pytest.mark.parametrize("cid", list(_RZ_BY_ID))
def test_redzone(cid):
    """the three runs of tests/test_abi_redzone_gpu.py::test_redzone over the entries of the second header: guards, exact
    workspaces, both fill bytes, a sibling case in between and a rerun"""
    c = _RZ_BY_ID[cid]
    a0, outs0 = rz._run(c, 0x00)
    v0 = rz._values(outs0)
    for o, got in zip(outs0, v0):
        if got.dtype.is_floating_point:
            assert bool(torch.isfinite(got).all()), f"{cid}: non-finite value in '{o.buf.name}' under fill 0x00"
        if o.ref is not None:
            rz._against(o, got, o.ref, f"{cid} fill 0x00")
    del a0
    a1, outs1 = rz._run(c, 0xFF)
    for o, got, first in zip(outs1, rz._values(outs1), v0):
        if got.dtype.is_floating_point:
            assert bool(torch.isfinite(got).all()), f"{cid}: non-finite value in '{o.buf.name}' under fill 0xFF"
        assert rz._bits_equal(got, first), f"{cid}: '{o.buf.name}' differs between fill 0x00 and fill 0xFF"
    del a1
    sib = REDZONE_CASES[(REDZONE_CASES.index(c) + 1) % len(REDZONE_CASES)]
    rz._run(sib, 0x00)
    a2, outs2 = rz._run(c, 0x00)
    for o, got, first in zip(outs2, rz._values(outs2), v0):
        assert rz._bits_equal(got, first), f"{cid}: '{o.buf.name}' changed after running {sib.id} in between"
