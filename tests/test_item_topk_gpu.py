"""Fused top-k inference head (csrc/item_topk.hip, ops.item_topk, torch.ops.t4r_hip.item_topk, NextItemPredictionTask
topk_mode): the k best items of alpha * X @ W^T per row without an [N, V] score matrix.

The comparator everywhere is the path that exists already and that the reference fixtures pin -- scores by the fp32-core
GEMM (ops.gemm under ops.precision("fp32")), then ops.topk -- and the fused result must equal it bit for bit: same values,
same ids, same order (value descending, ties to the lower index)."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _strided(t, extra):
    """the same values as a row-strided view with an odd pitch"""
    n, d = t.shape
    buf = torch.empty((n, d + extra), device=t.device, dtype=t.dtype)
    buf[:, :d] = t
    v = buf[:, :d]
    assert n == 1 or v.stride(0) % 2 == 1
    return v


def _inputs(N, V, D, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((N, D), generator=g)
    W = torch.randn((V, D), generator=g)
    return x, W


def _materialised(ops, x, W, k, alpha):
    with ops.precision("fp32"):
        return ops.topk(ops.gemm(x, W, False, True, alpha), k)


SHAPES = [(1, 7, 8, 7), (5, 301, 32, 10), (64, 5000, 64, 64), (300, 100001, 128, 20), (1024, 100001, 128, 256),
          (33, 65537, 100, 1), (130, 30011, 48, 100)]


@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("N,V,D,k", SHAPES)
def test_bit_equal_to_the_materialised_path(N, V, D, k, alpha):
    from transformers4rec_amd import ops

    x, W = _inputs(N, V, D, N + V + k)
    xd = _strided(x.to(DEV), 1 if D % 2 == 0 else 2)
    Wd = _strided(W.to(DEV), 3 if D % 2 == 0 else 2)
    calls = ops.item_topk_stats()["calls"]
    vals, ids = ops.item_topk(xd, Wd, k, alpha=alpha)
    st = ops.item_topk_stats()
    rv, ri = _materialised(ops, xd, Wd, k, alpha)
    print(f"[item_topk] N {N} V {V} D {D} k {k} alpha {alpha}: sample {st['sample_rows']} cap {st['list_capacity']} "
          f"fallback rows {st['fallback_rows']}")
    assert ids.dtype == torch.int64 and vals.dtype == torch.float32 and vals.shape == (N, k) and ids.shape == (N, k)
    assert torch.equal(ids, ri)
    assert torch.equal(vals, rv)
    assert st["calls"] == calls + 1
    assert st["fallback_rows"] == 0          # seeded Gaussian inputs: no row may need the overflow path


def test_default_precision_mode_does_not_change_the_result():
    """the fused head runs form 0 whatever the process-wide mode is"""
    from transformers4rec_amd import ops

    x, W = _inputs(200, 40000, 64, 11)
    xd, Wd = x.to(DEV), W.to(DEV)
    rv, ri = _materialised(ops, xd, Wd, 20, 1.0)
    for mode in ("auto", "fp32_bf16x3", "bf16"):
        with ops.precision(mode):
            v, i = ops.item_topk(xd, Wd, 20)
        assert torch.equal(i, ri) and torch.equal(v, rv), mode


def _stable_reference(ops, xd, Wd, k, alpha=1.0):
    with ops.precision("fp32"):
        s = ops.gemm(xd, Wd, False, True, alpha).cpu()
    order = torch.argsort(-s, dim=1, stable=True)[:, :k]
    return torch.gather(s, 1, order), order


def test_ties_duplicated_rows():
    from transformers4rec_amd import ops

    N, V, D, k = 40, 5000, 64, 20
    x, W = _inputs(N, V, D, 3)
    W[7] = W[3]
    W[V - 1] = W[V // 2]
    W[100:140] = W[50]                      # a tie group longer than k
    x[0] = W[3] * 3                         # row 0's best items are the tied pair 3 / 7
    x[1] = W[50] * 3                        # row 1's top-k is the tie group: lowest indices first
    xd, Wd = x.to(DEV), W.to(DEV)
    v, i = ops.item_topk(xd, Wd, k, alpha=0.5)
    rv, ri = _stable_reference(ops, xd, Wd, k, 0.5)
    assert torch.equal(i.cpu(), ri) and torch.equal(v.cpu(), rv)
    assert i[0, 0].item() == 3 and i[0, 1].item() == 7
    assert i[1, :k].tolist() == [50] + list(range(100, 100 + k - 1))


@pytest.mark.parametrize("case", ["constant_W", "zero_X", "3000_copies"])
@pytest.mark.parametrize("k", [10, 100])
def test_overflow_rows_take_the_materialised_path(case, k):
    from transformers4rec_amd import ops

    N, V, D = 70, 20011, 32
    x, W = _inputs(N, V, D, 5)
    if case == "constant_W":
        W[:] = 0.25
    elif case == "zero_X":
        x[:] = 0.0
        x[N - 1] = torch.randn(D, generator=torch.Generator().manual_seed(9))      # one ordinary row among them
    else:
        best = W[17].clone() * 4
        x[:] = best                                                    # every row's best item is 17 ...
        x += 0.01 * torch.randn((N, D), generator=torch.Generator().manual_seed(6))
        sel = torch.randperm(V, generator=torch.Generator().manual_seed(7))[:3000]
        W[sel] = best                                                  # ... and 3000 items are copies of it
    xd, Wd = x.to(DEV), W.to(DEV)
    v, i = ops.item_topk(xd, Wd, k)
    st = ops.item_topk_stats()
    rv, ri = _stable_reference(ops, xd, Wd, k)
    print(f"[item_topk overflow] {case} k {k}: fallback rows {st['fallback_rows']} of {N} (cap {st['list_capacity']})")
    assert torch.equal(i.cpu(), ri) and torch.equal(v.cpu(), rv)
    if case == "constant_W":
        assert st["fallback_rows"] == N
    elif case == "zero_X":
        assert st["fallback_rows"] == N - 1
    v2, i2 = ops.item_topk(xd, Wd, k)
    assert torch.equal(i, i2) and torch.equal(v, v2)


@pytest.mark.parametrize("table", ["fp32", "fp16", "bf16"])
def test_overflow_rows_with_gaps_between_them(table):
    """Six all-zero rows of x (every score tied at 0: more candidates than any list holds) among ordinary ones, as the runs
    {0, 1, 2}, {5}, {9, 10}: the overflow path recomputes runs of consecutive rows together and must split at the gaps.
    M = 1024 < V and cap = 2048 < V here, so exactly those six rows overflow (the others expect ~49 candidates).  Both heads
    go through the one driver (csrc/item_topk_plan.h: itk_run)."""
    from transformers4rec_amd import ops

    N, V, D, k = 12, 5000, 32, 10
    x, W = _inputs(N, V, D, 13)
    x[[0, 1, 2, 5, 9, 10]] = 0.0
    xd, Wd = x.to(DEV), W.to(DEV)
    if table == "fp32":
        rv, ri = _stable_reference(ops, xd, Wd, k)
    else:
        import test_item_topk_h16_gpu as h16

        Wd = ops.pack_item_table(Wd, table)
        rv, ri = h16._stable_reference(ops, xd, Wd, k)
    v, i = ops.item_topk(xd, Wd, k)
    st = ops.item_topk_stats()
    print(f"[item_topk overflow gaps] {table}: fallback rows {st['fallback_rows']} of {N} (sample {st['sample_rows']}, "
          f"cap {st['list_capacity']})")
    assert st["sample_rows"] < V and st["list_capacity"] < V
    assert st["fallback_rows"] == 6
    assert torch.equal(i.cpu(), ri) and torch.equal(v.cpu(), rv)
    v2, i2 = ops.item_topk(xd, Wd, k)
    assert torch.equal(i, i2) and torch.equal(v, v2)


# ------------------------------------------------------------------------------------------------ reference fixtures
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
        model.prediction_task.topk_mode = "fused"
    else:
        model.prediction_task.set_topk_mode("fused")
    x = {k[3:]: gu.t(v).to(DEV) for k, v in d.items() if k.startswith("in/")}
    return gu, e2e, d, model, x


@pytest.mark.parametrize("grad", [False, True], ids=["no_grad_operators", "grad_enabled_ctypes"])
@pytest.mark.parametrize("convert", [False, True], ids=["mirror", "dropin"])
@pytest.mark.parametrize("name,params_from,kw", INFER_FIXTURES)
def test_reference_fixtures_through_the_fused_head(name, params_from, kw, convert, grad):
    from transformers4rec_amd import ops

    gu, e2e, d, model, x = _fixture_model(name, params_from, kw, convert)
    model.top_k = 10
    calls = ops.item_topk_stats()["calls"]
    with torch.set_grad_enabled(grad):
        vals, ids = model(x)
    assert ops.item_topk_stats()["calls"] == calls + 1              # the fused head ran, not the materialised one
    rv, ri = torch.topk(gu.t(d["out/predictions"]), 10, dim=-1)
    assert torch.equal(ids.cpu(), ri)
    e2e.close(vals, rv)
    model.top_k = None                                              # top_k=None still returns the score matrix
    with torch.set_grad_enabled(grad):
        scores = model(x)
    e2e.close(scores, gu.t(d["out/predictions"]))


def test_task_constructor_argument_and_validation():
    import transformers4rec_amd as tr

    assert tr.NextItemPredictionTask(weight_tying=True).topk_mode == "auto"
    assert tr.NextItemPredictionTask(weight_tying=True, topk_mode="fused").topk_mode == "fused"
    with pytest.raises(ValueError):
        tr.NextItemPredictionTask(weight_tying=True, topk_mode="bogus")


# ------------------------------------------------------------------------------------------------ memory
def test_no_n_by_v_allocation():
    from transformers4rec_amd import ops

    N, V, D, k = 1024, 100001, 128, 20
    x, W = _inputs(N, V, D, 1)
    xd, Wd = x.to(DEV), W.to(DEV)
    ops.item_topk(xd, Wd, k)                                        # warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    v, i = ops.item_topk(xd, Wd, k)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    full = 4 * N * ops.pad_ld(V)
    print(f"[item_topk memory] peak extra {extra / 1e6:.1f} MB; the score matrix would be {full / 1e6:.1f} MB")
    assert extra < full / 4
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    _materialised(ops, xd, Wd, k, 1.0)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before >= 4 * N * V   # the comparator does hold the scores


# ------------------------------------------------------------------------------------------------ large vocabulary
def test_large_vocabulary_equals_materialised():
    from transformers4rec_amd import ops

    N, V, D, k = 256, 1000003, 64, 20
    g = torch.Generator(device=DEV).manual_seed(2)
    xd = torch.randn((N, D), device=DEV, generator=g)
    Wd = torch.randn((V, D), device=DEV, generator=g)
    v, i = ops.item_topk(xd, Wd, k)
    st = ops.item_topk_stats()
    rv, ri = _materialised(ops, xd, Wd, k, 1.0)
    assert torch.equal(i, ri) and torch.equal(v, rv)
    assert st["fallback_rows"] == 0
    v2, i2 = ops.item_topk(xd, Wd, k)
    assert torch.equal(i, i2) and torch.equal(v, v2)


def _tiny_task_model(V, L=20, D=64, topk_mode="auto"):
    import transformers4rec_amd as tr

    schema = tr.session_schema(V - 1, L)
    torch.manual_seed(0)
    inputs = tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=L, masking="mlm", embedding_dim_default=D)
    cfg = tr.XLNetConfig.build(D, 4, 1, total_seq_length=L, dropout=0.0)
    model = cfg.to_torch_model(inputs, tr.NextItemPredictionTask(weight_tying=True, topk_mode=topk_mode))
    return model.to(DEV).eval(), schema


@pytest.mark.parametrize("grad", [False, True], ids=["no_grad_operators", "grad_enabled_ctypes"])
def test_auto_mode_follows_the_head_size_limit(monkeypatch, grad):
    import transformers4rec_amd as tr
    from transformers4rec_amd import ops

    B, V, L = 256, 1000003, 20
    model, schema = _tiny_task_model(V)
    ids = tr.random_data_from_schema(schema, B, L, seed=3)["item_id"].to(DEV)
    model.top_k = 20
    assert 4 * B * ops.pad_ld(V) > 0.5 * (1 << 30)                  # 1 GB of scores
    with ops.precision("fp32"):         # body and materialised scores in form 0, so that both heads see the same hidden rows
        monkeypatch.delenv("T4R_HEAD_AUTO_GB", raising=False)
        calls = ops.item_topk_stats()["calls"]
        with torch.set_grad_enabled(grad):
            mv, mi = model({"item_id": ids})
        assert ops.item_topk_stats()["calls"] == calls              # default limit (4 GB): today's materialised path
        monkeypatch.setenv("T4R_HEAD_AUTO_GB", "0.5")
        with torch.set_grad_enabled(grad):
            fv, fi = model({"item_id": ids})
        assert ops.item_topk_stats()["calls"] == calls + 1          # above the limit: the fused head
    assert fv.shape == (B, 20) and fi.shape == (B, 20)
    assert torch.equal(fi, mi) and torch.equal(fv, mv)


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("N,V,D,k", [(1024, 100001, 128, 100), (77, 250007, 32, 10)])
def test_two_calls_give_identical_outputs(N, V, D, k):
    from transformers4rec_amd import ops

    x, W = _inputs(N, V, D, 21)
    xd, Wd = x.to(DEV), W.to(DEV)
    v1, i1 = ops.item_topk(xd, Wd, k, alpha=0.7)
    v2, i2 = ops.item_topk(xd, Wd, k, alpha=0.7)
    assert torch.equal(v1, v2) and torch.equal(i1, i2)


# ------------------------------------------------------------------------------------------------ operator
def test_operator_equals_the_ctypes_call_and_passes_opcheck():
    from transformers4rec_amd import ops, torch_ops  # noqa: F401

    x, W = _inputs(300, 30011, 64, 8)
    xd, Wd = x.to(DEV), W.to(DEV)
    v, i = torch.ops.t4r_hip.item_topk(xd, Wd, 0.5, 10)
    rv, ri = ops.item_topk(xd, Wd, 10, alpha=0.5)
    assert torch.equal(v, rv) and torch.equal(i, ri)
    torch.library.opcheck(torch.ops.t4r_hip.item_topk.default, (xd, Wd, 0.5, 10),
                          test_utils=("test_schema", "test_faketensor"))


def test_traced_inference_call_contains_the_node():
    from torch.fx.experimental.proxy_tensor import make_fx
    import transformers4rec_amd as tr
    from transformers4rec_amd import ops

    V, L, B = 3001, 20, 9
    model, schema = _tiny_task_model(V, topk_mode="fused")
    ids = tr.random_data_from_schema(schema, B, L, seed=4)["item_id"].to(DEV)
    task = model.prediction_task
    with torch.no_grad():
        h = model.transformer_block(model.input_features({"item_id": ids}))

        def f(hidden):
            return task(hidden, top_k=10)

        gm = make_fx(f)(h)
    targets = [str(nd.target) for nd in gm.graph.nodes if nd.op == "call_function"]
    assert any("t4r_hip.item_topk" in t for t in targets), targets
    assert not any("t4r_hip.item_scores" in t or "t4r_hip.topk" in t for t in targets), targets
    # (the last-position gather in front of the head is a direct library call, not an operator: the graph holds its result as
    # a constant, so the replay that is checked is the head's own -- the operator on its two operands)
    x, W = _inputs(50, 3001, 64, 4)
    xd, Wd = x.to(DEV), W.to(DEV)

    def g(a, b):
        return torch.ops.t4r_hip.item_topk(a, b, 0.5, 10)

    gm2 = make_fx(g)(xd, Wd)
    assert any("t4r_hip.item_topk" in str(nd.target) for nd in gm2.graph.nodes if nd.op == "call_function")
    (tv, ti), (ev, ei) = gm2(xd, Wd), ops.item_topk(xd, Wd, 10, alpha=0.5)
    assert torch.equal(ev, tv) and torch.equal(ei, ti)
