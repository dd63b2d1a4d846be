"""Inference head over a half-precision serving image of the item table (csrc/item_topk_h16.hip; ops.pack_item_table,
ops.item_scores / ops.item_topk with a 16-bit table, NextItemPredictionTask.prepare_serving).

Contract: score[n, v] = alpha * sum_d x16[n, d] * img[v, d], fp32 accumulation of exact products, x16 = x rounded to nearest
even in the image's dtype.  Every tolerance below is derived from that arithmetic, none is measured:
  * against fp64:  |s - ref| <= alpha * D * 2^-23 * (|x16| @ |img|^T) + 2^-23 * |ref|   (D fp32 additions of exact products, one ulp
    each whatever the cores' order or rounding mode, plus the multiplication by alpha);
  * against the same model's fp32 scores:  (2u + u^2) (|x| @ |W|^T) for the rounding of both operands (u = 2^-11 fp16, 2^-8 bf16),
    2 D 2^-23 (|x| @ |W|^T) for the two fp32 accumulations, 2^-14 (|x| @ sub(W)^T) for fp16 entries below 2^-14.
The fused head must equal topk(item_scores) bit for bit."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [("fp16", torch.float16), ("bf16", torch.bfloat16)]
U = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}
TINY16 = 2.0 ** -14                     # smallest normal fp16


def _strided(t, extra):
    n, d = t.shape
    buf = torch.empty((n, d + extra), device=t.device, dtype=t.dtype)
    buf[:, :d] = t
    return buf[:, :d]


def _inputs(N, V, D, seed, no_fp16_subnormals=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((N, D), generator=g)
    W = torch.randn((V, D), generator=g)
    if no_fp16_subnormals:              # |w| < 2^-14 is clamped up (sign kept; zeros stay): no fp16 subnormal operand anywhere
        for t in (x, W):
            small = (t.abs() < 2 * TINY16) & (t != 0)
            t[small] = torch.sign(t[small]) * 2 * TINY16
    return x, W


SHAPES = [(1, 7, 8, 7), (5, 301, 32, 10), (64, 5000, 64, 64), (300, 100001, 128, 20), (1024, 100001, 128, 256),
          (33, 65537, 100, 1), (130, 30011, 48, 100), (96, 20011, 512, 20), (40, 9001, 500, 10)]


# ------------------------------------------------------------------------------------------------ 1. pack
@pytest.mark.parametrize("name,td", DTYPES)
@pytest.mark.parametrize("V,D", [(1, 1), (7, 8), (301, 32), (5000, 100), (20011, 128), (3001, 500), (1000, 512)])
def test_pack_is_exact(name, td, V, D):
    from transformers4rec_amd import ops, torch_ops  # noqa: F401

    g = torch.Generator().manual_seed(V + D)
    W = torch.randn((V, D), generator=g) * torch.exp(3 * torch.randn((V, 1), generator=g))      # a few decades of magnitudes
    W = W.clamp(-6.0e4, 6.0e4)                                                                  # inside fp16's range
    W[0, 0] = 0.0
    if V > 5:
        W[3] *= 1e-6                                                                            # fp16 subnormals and zeros
    for Wd in (W.to(DEV), _strided(W.to(DEV), 3)):
        img = ops.pack_item_table(Wd, name)
        ldp = ops.image_ld(D)
        assert img.dtype == td and img.shape == (V, D) and (V == 1 or img.stride(0) == ldp) and img.stride(1) == 1
        assert ldp % 8 == 0 and ldp >= D and img.data_ptr() % 16 == 0
        assert torch.equal(img.view(torch.int16), Wd.to(td).view(torch.int16))                  # bit for bit: torch rounds to nearest even
        full = torch.as_strided(img, (V, ldp), (ldp, 1))
        assert bool((full[:, D:].view(torch.int16) == 0).all())                                 # pad columns are zero
    via_op = torch.ops.t4r_hip.pack_item_table(W.to(DEV), name)
    assert torch.equal(via_op.view(torch.int16), W.to(DEV).to(td).view(torch.int16))


@pytest.mark.parametrize("name,td", DTYPES)
def test_pack_refuses_a_table_that_does_not_round_to_finite_values(name, td):
    from transformers4rec_amd import ops

    W = torch.randn(50, 16)
    W[7, 3] = 3.0e38 if name == "bf16" else 7.0e4           # fp16 overflows above 65 504; bf16 keeps fp32's range: only inf / NaN
    if name == "bf16":
        W[7, 3] = float("inf")
    with pytest.raises(ValueError):
        ops.pack_item_table(W.to(DEV), name)


# ------------------------------------------------------------------------------------------------ 2. scores against fp64
def _score_bound(x16, img, alpha):
    ref = alpha * (x16.double() @ img.double().T)
    D = x16.shape[1]
    bound = alpha * D * 2.0 ** -23 * (x16.double().abs() @ img.double().abs().T) + 2.0 ** -23 * ref.abs()
    return ref, bound


@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("name,td", DTYPES)
@pytest.mark.parametrize("N,V,D,k", SHAPES)
def test_scores_against_fp64_with_the_derived_bound(N, V, D, k, name, td, alpha):
    from transformers4rec_amd import ops

    x, W = _inputs(N, V, D, N + V + k)
    xd = _strided(x.to(DEV), 1 if D % 2 == 0 else 2)
    img = ops.pack_item_table(W.to(DEV), name)
    s = ops.item_scores(xd, img, alpha)
    assert s.shape == (N, V) and s.dtype == torch.float32
    worst, slack = 0.0, float("inf")
    for r0 in range(0, N, 128):                              # fp64 reference in row blocks (memory)
        ref, bound = _score_bound(xd[r0:r0 + 128].to(td), img, alpha)
        err = (s[r0:r0 + 128].double() - ref).abs()
        worst = max(worst, float(err.max()))
        slack = min(slack, float((bound - err).min()))
        assert bool((err <= bound).all()), (name, float(err.max()), float((err - bound).max()))
    print(f"[scores h16] {name} N {N} V {V} D {D} alpha {alpha}: largest error {worst:.3e}, smallest bound - error {slack:.3e}")


def test_fp16_subnormal_operands():
    """Feeds fp16 SUBNORMAL table entries and prints what the matrix cores return.  Asserted is only the bound widened by
    2^-14 * sum |x16| over the subnormal entries (either behaviour -- honoured or flushed to zero -- passes).
    Observed on MI355X: HONOURED -- 130 940 subnormal entries, max |s - exact| 9.6e-6 with the plain bound violated at 0 of
    262 336 elements, max |s - flushed reference| 5.0e-4."""
    from transformers4rec_amd import ops

    N, V, D = 64, 4099, 128
    x, W = _inputs(N, V, D, 77)
    g = torch.Generator().manual_seed(78)
    sub_w = torch.rand((V, D), generator=g) < 0.25
    W[sub_w] = (torch.rand((V, D), generator=g)[sub_w] - 0.5) * TINY16            # |w| < 2^-15: subnormal in fp16
    xd = x.to(DEV)
    img = ops.pack_item_table(W.to(DEV), "fp16")
    x16 = xd.to(torch.float16)
    s = ops.item_scores(xd, img, 1.0).double()
    ref, bound = _score_bound(x16, img, 1.0)
    isub = (img.float().abs() < TINY16) & (img != 0)
    widen = TINY16 * (x16.double().abs() @ isub.double().T)          # a flushed entry loses at most 2^-14 |x16| per product
    flushed = x16.double() @ torch.where(isub, torch.zeros_like(img), img).double().T
    err, err_flushed = (s - ref).abs(), (s - flushed).abs()
    honoured = bool((err <= bound).all())
    print(f"[fp16 subnormals] {int(isub.sum())} table entries subnormal: max |s - exact| {float(err.max()):.3e} (plain bound "
          f"violated at {int((err > bound).sum())} of {err.numel()} elements), max |s - flushed reference| {float(err_flushed.max()):.3e}"
          f" -> subnormal operands {'HONOURED' if honoured else 'NOT honoured exactly (flushed or partly flushed)'}")
    assert bool((err <= bound + widen).all())


# ------------------------------------------------------------------------------------------------ 3. fused == materialised
def _check_fused(ops, xd, img, k, alpha, expect_no_fallback=None):
    calls = ops.item_topk_stats()["calls_h16"]
    v, i = ops.item_topk(xd, img, k, alpha=alpha)
    st = ops.item_topk_stats()
    rv, ri = ops.topk(ops.item_scores(xd, img, alpha), k)
    assert v.dtype == torch.float32 and i.dtype == torch.int64 and v.shape == rv.shape and i.shape == ri.shape
    assert torch.equal(i, ri)
    assert torch.equal(v.view(torch.int32), rv.view(torch.int32))
    assert st["calls_h16"] == calls + 1 and st["dtype"] == {torch.float16: "fp16", torch.bfloat16: "bf16"}[img.dtype]
    if expect_no_fallback:
        assert st["fallback_rows"] == 0
    return v, i, st


@pytest.mark.parametrize("name,td", DTYPES)
def test_smallest_shape_first(name, td):
    from transformers4rec_amd import ops

    x, W = _inputs(1, 7, 8, 15)
    _check_fused(ops, x.to(DEV), ops.pack_item_table(W.to(DEV), name), 7, 1.0, True)


@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("name,td", DTYPES)
@pytest.mark.parametrize("N,V,D,k", SHAPES)
def test_fused_equals_materialised_bit_for_bit(N, V, D, k, name, td, alpha):
    from transformers4rec_amd import ops

    x, W = _inputs(N, V, D, N + V + k)
    xd = _strided(x.to(DEV), 1 if D % 2 == 0 else 2)                 # row-strided x
    img = ops.pack_item_table(_strided(W.to(DEV), 3), name)
    v, i, st = _check_fused(ops, xd, img, k, alpha, True)
    print(f"[item_topk h16] {name} N {N} V {V} D {D} k {k} alpha {alpha}: sample {st['sample_rows']} cap {st['list_capacity']} "
          f"fallback rows {st['fallback_rows']}")
    # order: values descending, ties to the lower index
    assert bool((v[:, 1:] <= v[:, :-1]).all())
    tie = v[:, 1:] == v[:, :-1]
    assert bool((i[:, 1:][tie] > i[:, :-1][tie]).all())


def _stable_reference(ops, xd, img, k, alpha=1.0):
    s = ops.item_scores(xd, img, alpha).cpu()
    order = torch.argsort(-s, dim=1, stable=True)[:, :k]
    return torch.gather(s, 1, order), order


@pytest.mark.parametrize("name,td", DTYPES)
def test_ties_duplicated_rows(name, td):
    from transformers4rec_amd import ops

    N, V, D, k = 40, 5000, 64, 20
    x, W = _inputs(N, V, D, 3)
    W[7] = W[3]
    W[V - 1] = W[V // 2]
    W[100:140] = W[50]
    x[0] = W[3] * 3
    x[1] = W[50] * 3
    xd, img = x.to(DEV), ops.pack_item_table(W.to(DEV), name)
    v, i, _ = _check_fused(ops, xd, img, k, 0.5)
    rv, ri = _stable_reference(ops, xd, img, k, 0.5)
    assert torch.equal(i.cpu(), ri) and torch.equal(v.cpu(), rv)
    assert i[0, 0].item() == 3 and i[0, 1].item() == 7
    assert i[1, :k].tolist() == [50] + list(range(100, 100 + k - 1))


@pytest.mark.parametrize("name,td", DTYPES)
@pytest.mark.parametrize("case", ["constant_W", "zero_X", "3000_copies"])
@pytest.mark.parametrize("k", [10, 100])
def test_overflow_rows_take_the_materialised_path(case, k, name, td):
    from transformers4rec_amd import ops

    N, V, D = 70, 20011, 32
    x, W = _inputs(N, V, D, 5)
    if case == "constant_W":
        W[:] = 0.25
    elif case == "zero_X":
        x[:] = 0.0
        x[N - 1] = torch.randn(D, generator=torch.Generator().manual_seed(9))
    else:
        best = W[17].clone() * 4
        x[:] = best
        x += 0.01 * torch.randn((N, D), generator=torch.Generator().manual_seed(6))
        sel = torch.randperm(V, generator=torch.Generator().manual_seed(7))[:3000]
        W[sel] = best
    xd, img = x.to(DEV), ops.pack_item_table(W.to(DEV), name)
    v, i, st = _check_fused(ops, xd, img, k, 1.0)
    rv, ri = _stable_reference(ops, xd, img, k)
    print(f"[item_topk h16 overflow] {name} {case} k {k}: fallback rows {st['fallback_rows']} of {N} (cap {st['list_capacity']})")
    assert torch.equal(i.cpu(), ri) and torch.equal(v.cpu(), rv)
    if case == "constant_W":
        assert st["fallback_rows"] == N
    elif case == "zero_X":
        assert st["fallback_rows"] == N - 1
    v2, i2 = ops.item_topk(xd, img, k)
    assert torch.equal(i, i2) and torch.equal(v, v2)


@pytest.mark.parametrize("name,td", DTYPES)
def test_large_vocabulary_equals_materialised(name, td):
    from transformers4rec_amd import ops

    N, V, D, k = 256, 1000003, 64, 20
    g = torch.Generator(device=DEV).manual_seed(2)
    xd = torch.randn((N, D), device=DEV, generator=g)
    Wd = torch.randn((V, D), device=DEV, generator=g)
    img = ops.pack_item_table(Wd, name)
    v, i, st = _check_fused(ops, xd, img, k, 1.0, True)
    v2, i2 = ops.item_topk(xd, img, k)
    assert torch.equal(i, i2) and torch.equal(v, v2)


@pytest.mark.parametrize("name,td", DTYPES)
@pytest.mark.parametrize("N,V,D,k", [(1024, 100001, 128, 100), (77, 250007, 32, 10)])
def test_two_calls_give_identical_outputs(N, V, D, k, name, td):
    from transformers4rec_amd import ops

    x, W = _inputs(N, V, D, 21)
    xd, img = x.to(DEV), ops.pack_item_table(W.to(DEV), name)
    v1, i1 = ops.item_topk(xd, img, k, alpha=0.7)
    v2, i2 = ops.item_topk(xd, img, k, alpha=0.7)
    assert torch.equal(v1, v2) and torch.equal(i1, i2)


@pytest.mark.parametrize("name,td", DTYPES)
def test_no_n_by_v_allocation(name, td):
    from transformers4rec_amd import ops

    N, V, D, k = 1024, 100001, 128, 20
    x, W = _inputs(N, V, D, 1)
    xd, img = x.to(DEV), ops.pack_item_table(W.to(DEV), name)
    ops.item_topk(xd, img, k)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    v, i = ops.item_topk(xd, img, k)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    full = 4 * N * ops.pad_ld(V)
    print(f"[item_topk h16 memory] peak extra {extra / 1e6:.1f} MB; the score matrix would be {full / 1e6:.1f} MB")
    assert extra < full / 4


# ------------------------------------------------------------------------------------------------ 4. the fp32 path is untouched
def test_fp32_path_is_untouched_and_precision_mode_plays_no_part():
    from transformers4rec_amd import ops

    x, W = _inputs(200, 40000, 64, 11)
    xd, Wd = x.to(DEV), W.to(DEV)
    v0, i0 = ops.item_topk(xd, Wd, 20)
    assert ops.item_topk_stats()["dtype"] == "fp32"
    res = {}
    for name, td in DTYPES:
        img = ops.pack_item_table(Wd, name)
        res[name] = ops.item_topk(xd, img, 20)
        s0 = ops.item_scores(xd, img)
        for mode in ("auto", "fp32", "fp32_bf16x3", "bf16", "fp16"):
            with ops.precision(mode):
                v, i = ops.item_topk(xd, img, 20)
                s = ops.item_scores(xd, img)
            assert torch.equal(v, res[name][0]) and torch.equal(i, res[name][1]) and torch.equal(s, s0), (name, mode)
    v1, i1 = ops.item_topk(xd, Wd, 20)
    assert torch.equal(v0, v1) and torch.equal(i0, i1)
    with ops.precision("fp32"):
        rv, ri = ops.topk(ops.gemm(xd, Wd, False, True, 1.0), 20)
    assert torch.equal(v1, rv) and torch.equal(i1, ri)
    assert not torch.equal(res["fp16"][0], v0)              # and the 16-bit head is a different arithmetic, not an alias


# ------------------------------------------------------------------------------------------------ 5. task and drop-in
INFER_FIXTURES = [
    ("xlnet_mlm_item_infer", "xlnet_mlm_item_train", dict(emb_default=32)),
    ("xlnet_clm_item_infer", "xlnet_clm_item_train", dict(masking="clm", emb_default=32, weight_tying=False)),
    ("gpt2_clm_item_infer", "gpt2_clm_item_train", dict(masking="clm", emb_default=32, arch="gpt2")),
    ("bert_mlm_item_infer", "bert_mlm_item_train", dict(emb_default=32, arch="bert")),
    ("xlnet_mlm_long_infer", "xlnet_mlm_long_train", dict(emb_default=32)),
]


def _fixture_model(name, params_from, kw, convert=False):
    import golden_utils as gu
    import test_e2e_gpu as e2e
    import transformers4rec_amd as tr
    from transformers4rec_amd import dropin

    d = gu.load(name, params_from)
    model = e2e.build_model(d, **kw)
    e2e.load_reference_state(model, d)
    model.to(DEV).eval()
    if convert:
        ns = types.SimpleNamespace(TabularSequenceFeatures=tr.TabularSequenceFeatures, TransformerBlock=tr.TransformerBlock,
                                   NextItemPredictionTask=tr.NextItemPredictionTask)
        dropin.convert_model(model, ns)
        assert getattr(model.prediction_task, "_t4r_hip", False)
    x = {k[3:]: gu.t(v).to(DEV) for k, v in d.items() if k.startswith("in/")}
    return model, x


def _hidden_rows(ops, model, x, convert):
    """(xr, W, T): the last-position hidden rows exactly as the task forms them, its output weights and temperature"""
    from transformers4rec_amd.masking import MaskedLanguageModeling

    task = model.prediction_task
    seen = {}
    hook = task.register_forward_pre_hook(lambda m, a: seen.__setitem__("h", (a[0][0] if isinstance(a[0], (tuple, list)) else a[0]).detach()))
    with torch.no_grad():
        model(x)
    hook.remove()
    sh = task.hip_shadow() if convert else task
    h = seen["h"].float()
    B, Lg, D = h.shape
    pos = ops.last_positions(sh.embeddings.item_seq.contiguous(), Lg, isinstance(sh.masking, MaskedLanguageModeling), sh.padding_idx)
    xr = ops.gather_rows(h.contiguous().view(B * Lg, D), pos, B)
    if sh.task_block is not None:
        lin = sh.task_block[0][0]
        xr = ops.gemm(xr, lin.weight.detach(), False, True, bias=lin.bias.detach(), epilogue=ops.EPI_BIAS)
    mod = sh.pre.module
    T = float(mod.softmax_temperature) if mod.softmax_temperature else 1.0
    return xr, mod.output_weights.detach(), T


def _derived_tol(xr, W, T, name):
    """per row: max over items of the derived bound between the fp32 scores and the scores from the image (module docstring)"""
    u = U[name]
    D = xr.shape[1]
    aw = xr.double().abs() @ W.double().abs().T
    tol = (2 * u + u * u) * aw + 2 * D * 2.0 ** -23 * aw
    if name == "fp16":
        sub = (W.abs() < TINY16).double()
        tol = tol + TINY16 * (xr.double().abs() @ sub.T)
    return tol.max(dim=1).values / T


@pytest.mark.parametrize("grad", [False, True], ids=["no_grad_operators", "grad_enabled_ctypes"])
@pytest.mark.parametrize("convert", [False, True], ids=["mirror", "dropin"])
@pytest.mark.parametrize("name,td", DTYPES)
@pytest.mark.parametrize("fixture,params_from,kw", INFER_FIXTURES)
def test_task_and_dropin_serve_from_the_image(fixture, params_from, kw, name, td, convert, grad):
    from transformers4rec_amd import ops

    model, x = _fixture_model(fixture, params_from, kw, convert)
    task = model.prediction_task
    keys = list(model.state_dict().keys())
    assert task.serving_dtype is None
    with ops.precision("fp32"):
        model.top_k = None
        with torch.set_grad_enabled(grad):
            S = model(x).clone()                                     # the same model's own fp32 scores
            model.top_k = 10
            v_before, i_before = model(x)
        xr, W, T = _hidden_rows(ops, model, x, convert)
        packs = task.serving_packs
        assert task.prepare_serving(name) is task and task.serving_dtype == name and task.serving_packs == packs + 1
        assert list(model.state_dict().keys()) == keys
        calls = ops.item_topk_stats()["calls_h16"]
        with torch.set_grad_enabled(grad):
            vals, ids = model(x)
        st = ops.item_topk_stats()
        assert st["calls_h16"] == calls + 1 and st["dtype"] == name           # the 16-bit head ran
        assert task.serving_packs == packs + 1                                 # nothing re-packed
        ev, ei = ops.item_topk(xr, ops.pack_item_table(W, name), 10, 1.0 / T)
        assert torch.equal(ids, ei) and torch.equal(vals.view(torch.int32), ev.view(torch.int32))
        tol = _derived_tol(xr, W, T, name)
        Sd = S.double()
        got = torch.gather(Sd, 1, ids)
        kth = torch.topk(Sd, 10, dim=1).values[:, -1]
        dv = (vals.double() - got).abs()
        print(f"[serving {name}] {fixture}: max |vals - S[ids]| {float(dv.max()):.3e}, smallest tol {float(tol.min()):.3e}; "
              f"ids equal to fp32 top-10 in {int((ids == i_before).all(dim=1).sum())} of {ids.shape[0]} rows")
        assert bool((dv <= tol[:, None]).all())
        assert bool((got >= (kth - 2 * tol)[:, None]).all())
        model.top_k = None
        with torch.set_grad_enabled(grad):
            scores = model(x)
        assert scores.shape == S.shape and scores.dtype == torch.float32
        assert bool(((scores.double() - Sd).abs() <= tol[:, None]).all())
        assert torch.equal(scores, ops.item_scores(xr, ops.pack_item_table(W, name), 1.0 / T))
        task.drop_serving_image()
        assert task.serving_dtype is None
        with torch.set_grad_enabled(grad):
            assert torch.equal(model(x), S)
            model.top_k = 10
            v_after, i_after = model(x)
        assert torch.equal(v_after, v_before) and torch.equal(i_after, i_before)
        assert list(model.state_dict().keys()) == keys


# ------------------------------------------------------------------------------------------------ 6. never stale
def _tiny_task_model(V, L=20, D=64):
    import transformers4rec_amd as tr

    schema = tr.session_schema(V - 1, L)
    torch.manual_seed(0)
    inputs = tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=L, masking="mlm", embedding_dim_default=D)
    cfg = tr.XLNetConfig.build(D, 4, 1, total_seq_length=L, dropout=0.0)
    model = cfg.to_torch_model(inputs, tr.NextItemPredictionTask(weight_tying=True))
    return model.to(DEV), schema


def _task_rows(ops, model, ids):
    from transformers4rec_amd.masking import MaskedLanguageModeling

    task = model.prediction_task
    with torch.no_grad():
        h = model.transformer_block(model.input_features({"item_id": ids})).float()
    B, Lg, D = h.shape
    pos = ops.last_positions(task.embeddings.item_seq.contiguous(), Lg, isinstance(task.masking, MaskedLanguageModeling),
                             task.padding_idx)
    return ops.gather_rows(h.contiguous().view(B * Lg, D), pos, B)


@pytest.mark.parametrize("name,td", DTYPES)
def test_the_image_is_never_served_stale(name, td):
    import transformers4rec_amd as tr
    from transformers4rec_amd import ops

    V, L, B = 3001, 20, 32
    model, schema = _tiny_task_model(V)
    task = model.prediction_task
    ids = tr.random_data_from_schema(schema, B, L, seed=4)["item_id"].to(DEV)
    dense, tables = tr.flatten_model(model)
    opt = tr.FusedAdam([dense, tables], lr=5e-2)
    model.eval()
    model.top_k = 10
    task.prepare_serving(name)
    packs = task.serving_packs
    with torch.no_grad():
        v0, i0 = model({"item_id": ids})
        v0b, i0b = model({"item_id": ids})
    assert task.serving_packs == packs                          # two inference calls in a row pack nothing
    assert torch.equal(v0, v0b) and torch.equal(i0, i0b)
    old_image = task._serving_image.clone()

    # one training step: FusedAdam writes the flat buffers through raw pointers
    model.train()
    tdata = tr.random_data_from_schema(schema, B, L, seed=5)["item_id"].to(DEV)
    model({"item_id": tdata}, training=True)["loss"].backward()
    opt.step()
    model.eval()
    with torch.no_grad():
        v1, i1 = model({"item_id": ids})
    assert task.serving_dtype == name and task.serving_packs == packs + 1
    W = task.pre.module.output_weights.detach()
    xr = _task_rows(ops, model, ids)
    T = float(task.pre.module.softmax_temperature) if task.pre.module.softmax_temperature else 1.0
    ev, ei = ops.item_topk(xr, ops.pack_item_table(W, name), 10, 1.0 / T)
    assert torch.equal(v1, ev) and torch.equal(i1, ei)
    sv, si = ops.item_topk(xr, old_image, 10, 1.0 / T)          # what a stale image would have served
    assert not (torch.equal(v1, sv) and torch.equal(i1, si))
    with torch.no_grad():
        model({"item_id": ids})
    assert task.serving_packs == packs + 1

    # load_state_dict of perturbed weights
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    g = torch.Generator(device=DEV).manual_seed(9)
    for k, v in sd.items():
        if v.is_floating_point():
            sd[k] = v * (1.0 + 0.2 * torch.randn(v.shape, device=v.device, generator=g))
    old_image = task._serving_image.clone()
    model.load_state_dict(sd)
    with torch.no_grad():
        v2, i2 = model({"item_id": ids})
    assert task.serving_dtype == name and task.serving_packs == packs + 2
    W = task.pre.module.output_weights.detach()
    xr = _task_rows(ops, model, ids)
    ev, ei = ops.item_topk(xr, ops.pack_item_table(W, name), 10, 1.0 / T)
    assert torch.equal(v2, ev) and torch.equal(i2, ei)
    sv, si = ops.item_topk(xr, old_image, 10, 1.0 / T)
    assert not (torch.equal(v2, sv) and torch.equal(i2, si))
    with torch.no_grad():
        model({"item_id": ids})
    assert task.serving_packs == packs + 2


# ------------------------------------------------------------------------------------------------ 7. operator
@pytest.mark.parametrize("name,td", DTYPES)
def test_operator_equals_the_ctypes_call_and_passes_opcheck(name, td):
    from transformers4rec_amd import ops, torch_ops  # noqa: F401

    x, W = _inputs(300, 30011, 64, 8)
    xd, img = x.to(DEV), ops.pack_item_table(W.to(DEV), name)
    v, i = torch.ops.t4r_hip.item_topk(xd, img, 0.5, 10)
    rv, ri = ops.item_topk(xd, img, 10, alpha=0.5)
    assert torch.equal(v, rv) and torch.equal(i, ri)
    assert torch.equal(torch.ops.t4r_hip.item_scores(xd, img, 0.5), ops.item_scores(xd, img, 0.5))
    torch.library.opcheck(torch.ops.t4r_hip.item_topk.default, (xd, img, 0.5, 10), test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.t4r_hip.item_scores.default, (xd, img, 0.5), test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.t4r_hip.pack_item_table.default, (W.to(DEV), name), test_utils=("test_schema", "test_faketensor"))


@pytest.mark.parametrize("name,td", DTYPES)
def test_traced_inference_call_contains_the_node(name, td):
    from torch.fx.experimental.proxy_tensor import make_fx
    import transformers4rec_amd as tr
    from transformers4rec_amd import ops

    V, L, B = 3001, 20, 9
    model, schema = _tiny_task_model(V)
    model.eval()
    ids = tr.random_data_from_schema(schema, B, L, seed=4)["item_id"].to(DEV)
    task = model.prediction_task
    task.prepare_serving(name)
    with torch.no_grad():
        h = model.transformer_block(model.input_features({"item_id": ids}))
        ev, ei = task(h, top_k=10)

        def f(hidden):
            return task(hidden, top_k=10)

        gm = make_fx(f)(h)
    nodes = [nd for nd in gm.graph.nodes if nd.op == "call_function" and "t4r_hip.item_topk" in str(nd.target)]
    assert len(nodes) == 1, [str(nd.target) for nd in gm.graph.nodes]
    targets = [str(nd.target) for nd in gm.graph.nodes if nd.op == "call_function"]
    assert not any("t4r_hip.item_scores" in t or "t4r_hip.topk" in t for t in targets), targets
    img = ops.pack_item_table(task.pre.module.output_weights.detach(), name)

    def g(a, b):
        return torch.ops.t4r_hip.item_topk(a, b, 0.5, 10)

    x, _ = _inputs(50, V, 64, 4)
    xd = x.to(DEV)
    gm2 = make_fx(g)(xd, img)
    (tv, ti), (rv, ri) = gm2(xd, img), ops.item_topk(xd, img, 10, alpha=0.5)
    assert torch.equal(rv, tv) and torch.equal(ri, ti)
