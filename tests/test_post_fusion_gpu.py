"""Post-context fusion on the GPU: the kernels (csrc/post_fusion.hip, include/t4r_hip_postfusion.h) against float64
(tests/post_fusion_restatement.py) under its per-element bounds, the scalar path of unaligned operands, bit equality across launch
shapes and runs, accumulation, red zones around every buffer with an exact workspace; the registered operator; and the
PostContextFusion module around a body: one training step against the reference's fixtures
(tests/golden/post_fusion_{mul,sum,concat}_train.npz, tools/make_post_fusion_golden.py) at the tolerances of tests/test_e2e_gpu.py, both
gradient modes, the fused optimizer, evaluation.

Every numeric test prints the largest observed error / bound ratio; with T4R_RATIO_LOG set to a path the maxima over the run are
also written there as text: profiles/post_fusion_margins.txt is that file."""
import atexit
import os

import pytest
import torch

import post_fusion_restatement as R
import transformers4rec_amd as tr
from abi_arena import FILLS, Arena
from transformers4rec_amd import _lib, ops, torch_ops  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32

BL = [(1, 1), (3, 7), (5, 13), (13, 20)]            # T = 1, 21, 65, 260: below a wave, below / above a 64-token split, three workgroups
DS = [64, 100, 128, 320]                            # whole 32-row tiles, a ragged last tile (100 = 3 x 32 + 4), ten tiles
CS = [1, 24, 65, 256]                               # one step with an empty slot, C % 4 == 0, C % 4 == 1 over two c tiles, the limit
RATIOS = {}


def _note(what, ratio):
    RATIOS[what] = max(RATIOS.get(what, 0.0), float(ratio))


MARGINS_HEAD = """Post-context fusion (csrc/post_fusion.hip): worst error / bound per quantity on an MI355X
Written by tests/test_post_fusion_gpu.py:  T4R_RATIO_LOG=profiles/post_fusion_margins.txt pytest -m gpu tests/test_post_fusion_gpu.py
Kernel level (out/, dseq/, dctx/, d_w/, d_b/): the bounds of tests/post_fusion_restatement.py over the shapes of the test.
model/: the Model with fusion against the restated fusion of its own body output and context, same bounds.
fixture/<aggregation>/<quantity>: the Model with fusion against the reference's training step (tests/golden/post_fusion_*_train.npz),
|got - want| / (atol + rtol |want|) with the tolerances tests/test_e2e_gpu.py applies to xlnet_clm_item_train.
A ratio of 0 is bit equality.
"""


@atexit.register
def _dump_ratios():
    path = os.environ.get("T4R_RATIO_LOG")
    if path and RATIOS:
        with open(path, "w") as f:
            f.write(MARGINS_HEAD + "\n")
            for k in sorted(RATIOS):
                f.write(f"{k:<60s} {RATIOS[k]:.4f}\n")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(k):
    return {n: v.to(DEV) for n, v in k.items()}


def _run(k, mode, accumulate=False):
    """forward and backward of one case through ops -> (out, grads dict), host tensors"""
    d = _dev(k)
    m = R.MODE_ID[mode]
    W, b = (None, None) if mode == "concat" else (d["W"], d["b"])
    out = ops.post_fusion_fwd(d["seq"], d["ctx"], W, b, m)
    dout = d["dout_cat"] if mode == "concat" else d["dout"]
    d_w = d_b = None
    if mode != "concat":
        d_w = d["d_w0"].clone() if accumulate else torch.zeros_like(d["W"])
        d_b = d["d_b0"].clone() if accumulate else torch.zeros_like(d["b"])
    dseq, dctx = ops.post_fusion_bwd_(dout, d["seq"], d["ctx"], W, b, m, d_w, d_b)
    grads = {"dseq": dseq.cpu(), "dctx": dctx.cpu()}
    if mode != "concat":
        grads.update(d_w=d_w.cpu(), d_b=d_b.cpu())
    return out.cpu(), grads


def _check(tag, k, mode, out, grads, accumulate=False):
    want, bound = R.forward(k["seq"], k["ctx"], k["W"], k["b"], mode)
    r = R.ratio(out, want, bound)
    _note(f"out/{mode}", r)
    worst = {"out": r}
    assert r <= 1.0, (tag, mode, "out", r)
    dout = k["dout_cat"] if mode == "concat" else k["dout"]
    ref = R.gradients(dout, k["seq"], k["ctx"], k["W"], k["b"], mode, k["d_w0"] if accumulate else None,
                      k["d_b0"] if accumulate else None)
    session = "session" if k["ctx"].dim() == 2 else "sequence"
    for name, (val, bnd) in ref.items():
        r = R.ratio(grads[name].reshape(val.shape), val, bnd)
        _note(f"{name}/{mode}" + (f"/{session}" if name == "dctx" else ""), r)
        worst[name] = r
        assert r <= 1.0, (tag, mode, name, r)
    return worst


# ------------------------------------------------------------------------------------------------ entries against float64
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("B,L", BL)
def test_entries_against_float64(B, L, D):
    """every C, the three modes, both context ranks and magnitudes 1 and 30: each output within its bound; concat and the dseq of
    elementwise-sum are the inputs' bits"""
    for C in CS:
        for session in (False, True):
            for scale in (1.0, 30.0):
                k = R.make_case(B, L, D, C, session, scale)
                for mode in R.MODES:
                    out, grads = _run(k, mode)
                    tag = (B, L, D, C, session, scale)
                    worst = _check(tag, k, mode, out, grads)
                    print(f"{tag} {mode}: " + ", ".join(f"{n} {v:.3f}" for n, v in worst.items()))
                    if mode == "concat":
                        x = k["ctx"].unsqueeze(1).expand(-1, L, -1) if session else k["ctx"]
                        assert torch.equal(out, torch.cat([k["seq"], x], dim=-1))
                        assert torch.equal(grads["dseq"], k["dout_cat"][..., :D])
                        if not session or L == 1:
                            assert torch.equal(grads["dctx"].reshape(B, L, C), k["dout_cat"][..., D:])
                    if mode == "sum":
                        assert torch.equal(grads["dseq"], k["dout"])


def test_planted_faults_exceed_the_bounds_at_the_gpu_shapes():
    """the bounds have teeth at the shapes above: each planted fault of the restatement is far outside"""
    k = R.make_case(5, 13, 100, 65, True)
    out, bound = R.forward(k["seq"], k["ctx"], k["W"], k["b"], "mul")
    for fault in ("no_one_plus", "no_bias", "c_truncated", "session_row_mod"):
        bad, _ = R.forward(k["seq"], k["ctx"], k["W"], k["b"], "mul", fault=fault)
        assert R.ratio(bad.float(), out, bound) > 100.0, fault


# ------------------------------------------------------------------------------------------------ unaligned operands
@pytest.mark.parametrize("mode,which", [(m, w) for m in R.MODES for w in ("seq", "ctx", "W", "dout") if (m, w) != ("concat", "W")])
def test_a_view_at_a_4_byte_offset_takes_the_scalar_path_with_the_same_bits(mode, which):
    k = _dev(R.make_case(5, 13, 128, 24, False))
    m = R.MODE_ID[mode]

    def run(kk):
        W, b = (None, None) if mode == "concat" else (kk["W"], kk["b"])
        dout = kk["dout_cat"] if mode == "concat" else kk["dout"]
        out = ops.post_fusion_fwd(kk["seq"], kk["ctx"], W, b, m)
        d_w = None if W is None else torch.zeros_like(k["W"])
        d_b = None if W is None else torch.zeros_like(k["b"])
        dseq, dctx = ops.post_fusion_bwd_(dout, kk["seq"], kk["ctx"], W, b, m, d_w, d_b)
        return [out, dseq, dctx] + ([] if W is None else [d_w, d_b])

    name = "dout_cat" if (which == "dout" and mode == "concat") else which
    shifted = dict(k)
    flat = torch.empty(k[name].numel() + 1, device=DEV)
    view = flat[1:].view(k[name].shape)
    view.copy_(k[name])
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    shifted[name] = view
    for a, b in zip(run(k), run(shifted)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ bit equality
@pytest.mark.parametrize("session", [False, True], ids=["sequence", "session"])
@pytest.mark.parametrize("mode", ["mul", "sum"])
def test_a_row_has_the_same_bits_alone_and_in_a_batch(mode, session):
    k = _dev(R.make_case(13, 20, 100, 65, session))
    m = R.MODE_ID[mode]
    full = ops.post_fusion_fwd(k["seq"], k["ctx"], k["W"], k["b"], m)
    full_dseq, _ = ops.post_fusion_bwd_(k["dout"], k["seq"], k["ctx"], k["W"], k["b"], m, want_dctx=False)
    for bi, li in ((0, 0), (7, 13), (12, 19)):
        ctx1 = k["ctx"][bi:bi + 1].contiguous() if session else k["ctx"][bi:bi + 1, li:li + 1].contiguous()
        seq1, dout1 = k["seq"][bi:bi + 1, li:li + 1].contiguous(), k["dout"][bi:bi + 1, li:li + 1].contiguous()
        one = ops.post_fusion_fwd(seq1, ctx1, k["W"], k["b"], m)                      # T = 1
        assert torch.equal(one[0, 0], full[bi, li])
        one_dseq, _ = ops.post_fusion_bwd_(dout1, seq1, ctx1, k["W"], k["b"], m, want_dctx=False)
        assert torch.equal(one_dseq[0, 0], full_dseq[bi, li])


@pytest.mark.parametrize("session", [False, True], ids=["sequence", "session"])
@pytest.mark.parametrize("mode", ["mul", "sum"])
def test_two_runs_give_the_same_bits_and_gradients_accumulate(mode, session):
    k = R.make_case(13, 20, 100, 65, session, seed=1)
    _, g1 = _run(k, mode)
    _, g2 = _run(k, mode)
    for name in ("d_w", "d_b", "dctx", "dseq"):
        assert torch.equal(g1[name], g2[name]), name
    # accumulated: the batch sum is formed first, then added once to what the buffers held
    out, g3 = _run(k, mode, accumulate=True)
    assert torch.equal(g3["d_w"], k["d_w0"] + g1["d_w"]) and torch.equal(g3["d_b"], k["d_b0"] + g1["d_b"])
    assert torch.equal(g3["dctx"], g1["dctx"]) and torch.equal(g3["dseq"], g1["dseq"])          # overwritten, not accumulated
    _check("accumulate", k, mode, out, g3, accumulate=True)


def test_null_outputs_and_no_tokens():
    k = _dev(R.make_case(3, 7, 64, 24, True))
    d_w = torch.zeros_like(k["W"])
    full_w, full_b = torch.zeros_like(k["W"]), torch.zeros_like(k["b"])
    dseq, dctx = ops.post_fusion_bwd_(k["dout"], k["seq"], k["ctx"], k["W"], k["b"], 0, full_w, full_b)
    only_w = ops.post_fusion_bwd_(k["dout"], k["seq"], k["ctx"], k["W"], k["b"], 0, d_w, None, want_dseq=False, want_dctx=False)
    assert only_w == (None, None) and torch.equal(d_w, full_w)
    only_ctx = ops.post_fusion_bwd_(k["dout"], k["seq"], k["ctx"], k["W"], k["b"], 0, want_dseq=False)
    assert only_ctx[0] is None and torch.equal(only_ctx[1], dctx)
    only_seq = ops.post_fusion_bwd_(k["dout"], k["seq"], k["ctx"], k["W"], k["b"], 0, want_dctx=False)
    assert only_seq[1] is None and torch.equal(only_seq[0], dseq)
    empty = ops.post_fusion_fwd(k["seq"][:0], k["ctx"][:0], k["W"], k["b"], 0)
    assert empty.shape == (0, 7, 64)


# ------------------------------------------------------------------------------------------------ buffer discipline
@pytest.mark.parametrize("fill", FILLS, ids=["zeros", "ones"])
@pytest.mark.parametrize("session", [False, True], ids=["sequence", "session"])
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("B,L,D,C", [(5, 13, 100, 65), (13, 20, 64, 24)])
def test_red_zones_around_every_buffer(B, L, D, C, mode, session, fill):
    """guards around every buffer, the workspace exactly as large as the size query says, under both fills, each call twice"""
    lib = _lib.load()
    k = R.make_case(B, L, D, C, session)
    T, m, ps = B * L, R.MODE_ID[mode], int(session)
    Do = D + C if mode == "concat" else D
    assert lib.t4r_post_fusion_supported(D, C) == 1
    a = Arena(fill, DEV, capacity=16 << 20)
    seq = a.new("seq", "in", F32, T * D).set(k["seq"])
    ctx = a.new("ctx", "in", F32, k["ctx"].numel()).set(k["ctx"])
    Wb = a.new("W", "in", F32, D * C).set(k["W"])
    bb = a.new("b", "in", F32, D).set(k["b"])
    out = a.new("out", "out", F32, T * Do)
    a.seal()
    Wp, bp = (None, None) if mode == "concat" else (Wb.ptr, bb.ptr)
    want = ops.post_fusion_fwd(k["seq"].to(DEV), k["ctx"].to(DEV), *((None, None) if mode == "concat" else (k["W"].to(DEV), k["b"].to(DEV))), m)
    for _ in range(2):
        rc = lib.t4r_post_fusion_fwd(_stream(), seq.ptr, ctx.ptr, Wp, bp, out.ptr, T, L, D, C, m, ps)
        assert rc == 0, lib.t4r_last_error()
        torch.cuda.synchronize()
        v = a.check()
        assert v is None, str(v)
        assert a.nonfinite() is None
        assert torch.equal(out.t.view(B, L, Do), want)
    # ---- backward: the exact workspace
    dY = k["dout_cat"] if mode == "concat" else k["dout"]
    dyb = a.new("dout", "in", F32, T * Do).set(dY)
    dseq = a.new("dseq", "out", F32, T * D)
    dctx = a.new("dctx", "out", F32, k["ctx"].numel())
    dW = a.new("d_w", "inout", F32, D * C).set(0)
    db = a.new("d_b", "inout", F32, D).set(0)
    n_ws = lib.t4r_post_fusion_bwd_ws_floats(T, L, D, C, m, ps)
    assert (n_ws == 0) == (mode == "concat")
    ws = a.ws("ws", 4 * n_ws)
    a.seal()
    dWp, dbp = (None, None) if mode == "concat" else (dW.ptr, db.ptr)
    first = None
    for _ in range(2):
        if mode != "concat":
            dW.t.zero_()
            db.t.zero_()
        rc = lib.t4r_post_fusion_bwd(_stream(), dyb.ptr, seq.ptr, ctx.ptr, Wp, bp, dseq.ptr, dctx.ptr, dWp, dbp,
                                     ws.ptr if n_ws else None, T, L, D, C, m, ps)
        assert rc == 0, lib.t4r_last_error()
        torch.cuda.synchronize()
        v = a.check()
        assert v is None, str(v)
        assert a.nonfinite() is None
        got = [dseq.bits(), dctx.bits()] + ([] if mode == "concat" else [dW.bits(), db.bits()])
        if first is None:
            first = got
        for x, y in zip(first, got):
            assert torch.equal(x, y)
    grads = {"dseq": dseq.t.view(B, L, D).cpu(), "dctx": dctx.t.view(k["ctx"].shape).cpu()}
    if mode != "concat":
        grads.update(d_w=dW.t.view(D, C).cpu(), d_b=db.t.cpu())
    _check("arena", k, mode, out.t.view(B, L, Do).cpu(), grads)


# ------------------------------------------------------------------------------------------------ registered operator
@pytest.mark.parametrize("mode", R.MODES)
def test_registered_operator_equals_the_ctypes_call_and_differentiates(mode):
    k = _dev(R.make_case(3, 7, 64, 24, True))
    m = R.MODE_ID[mode]
    W, b = (None, None) if mode == "concat" else (k["W"].clone().requires_grad_(), k["b"].clone().requires_grad_())
    seq, ctx = k["seq"].clone().requires_grad_(), k["ctx"].clone().requires_grad_()
    out = torch.ops.t4r_hip.post_fusion(seq, ctx, W, b, m)
    want = ops.post_fusion_fwd(k["seq"], k["ctx"], None if W is None else k["W"], None if b is None else k["b"], m)
    assert torch.equal(out, want)
    dout = k["dout_cat"] if mode == "concat" else k["dout"]
    out.backward(dout)
    d_w = None if W is None else torch.zeros_like(k["W"])
    d_b = None if W is None else torch.zeros_like(k["b"])
    dseq, dctx = ops.post_fusion_bwd_(dout, k["seq"], k["ctx"], None if W is None else k["W"], None if b is None else k["b"], m, d_w, d_b)
    assert torch.equal(seq.grad, dseq) and torch.equal(ctx.grad, dctx)
    if W is not None:
        assert torch.equal(W.grad, d_w) and torch.equal(b.grad, d_b)


# ------------------------------------------------------------------------------------------------ module level
V, L, D, B = 50, 20, 64, 13
AGGREGATIONS = ("elementwise-mul", "elementwise-sum", "concat")
MODE_OF = {"elementwise-mul": "mul", "elementwise-sum": "sum", "concat": "concat"}


def _model(aggregation, context, seed=0):
    """XLNet d 64, 2 layers, 4 heads, L 20, CLM, tied head, with a session-level (EmbeddingFeatures) or sequence-level
    (SequenceEmbeddingFeatures) context of 24 columns"""
    torch.manual_seed(seed)
    feats = tr.TabularSequenceFeatures.from_schema(tr.session_schema(V, L), max_sequence_length=L, masking="clm",
                                                   aggregation="concat", embedding_dims={"item_id": D})
    cfg = tr.XLNetConfig.build(d_model=D, n_head=4, n_layer=2, total_seq_length=L, dropout=0.0)
    block = tr.TransformerBlock(cfg, masking=feats.masking)
    if context == "session":
        ctx = tr.EmbeddingFeatures({"user": tr.FeatureConfig(tr.TableConfig(11, 8, name="user")),
                                    "country": tr.FeatureConfig(tr.TableConfig(7, 16, name="country"))}, aggregation="concat")
    elif context == "tabular":      # a TabularSequenceFeatures without masking, with tables of its own: item 16 | category 8 wide
        ctx = tr.TabularSequenceFeatures.from_schema(tr.session_schema(V, L, categoricals=(("category", 12),)), max_sequence_length=L,
                                                     aggregation="concat", embedding_dims={"item_id": 16, "category": 8})
    else:
        ctx = tr.SequenceEmbeddingFeatures({"category": (13, 24)}, aggregation="concat")
    model = tr.Model(feats, block, tr.NextItemPredictionTask(weight_tying=True), post_context_module=ctx,
                     fusion_aggregation=aggregation)
    return model.to(DEV)


def _batch(context):
    g = torch.Generator().manual_seed(5)
    lens = torch.randint(5, L + 1, (B,), generator=g)
    lens[0] = L
    m = torch.arange(L)[None] < lens[:, None]
    x = {"item_id": (torch.randint(1, V + 1, (B, L), generator=g) * m).to(DEV)}
    if context == "session":
        x["user"] = torch.randint(0, 11, (B,), generator=g).to(DEV)
        x["country"] = torch.randint(0, 7, (B,), generator=g).to(DEV)
    else:
        x["category"] = (torch.randint(1, 13, (B, L), generator=g) * m).to(DEV)
    return x


def _context_table(model, context):
    tabs = model.heads[0].body.post_context_module.embedding_tables
    return tabs["user" if context == "session" else "category"].weight


# ------------------------------------------------------------------------------------------------ against the reference's step
FIXTURES = {"post_fusion_mul_train": "mul", "post_fusion_sum_train": "sum", "post_fusion_concat_train": "concat"}
BODY = "heads.0.body."


def _fixture_model(d):
    """the mirror of tools/make_post_fusion_golden.py's reference model, with the reference's parameters"""
    import test_e2e_gpu as e2e

    Lf, Vf, Df = int(d["meta/L"]), int(d["meta/V"]), int(d["meta/d_model"])
    feats = tr.TabularSequenceFeatures.from_schema(tr.session_schema(Vf - 1, Lf), max_sequence_length=Lf, masking="clm",
                                                   aggregation="concat", embedding_dims={"item_id": int(d["meta/d_item"])})
    cfg = tr.XLNetConfig.build(d_model=Df, n_head=int(d["meta/n_head"]), n_layer=int(d["meta/n_layer"]), total_seq_length=Lf, dropout=0.0)
    ctx = tr.SequenceEmbeddingFeatures({"category": (int(d["meta/cat_card"]) + 1, int(d["meta/cat_dim"]))}, aggregation="concat")
    model = tr.Model(feats, tr.TransformerBlock(cfg, masking=feats.masking), tr.NextItemPredictionTask(weight_tying=True),
                     post_context_module=ctx, fusion_aggregation=str(d["meta/fusion_aggregation"]))
    e2e.load_reference_state(model, d)
    return model.to(DEV)


def _tol_ratio(got, want, tol):
    got, want = got.detach().cpu().double(), want.double()
    return float(((got - want).abs() / (tol["atol"] + tol["rtol"] * want.abs())).max())


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_train_step_matches_the_reference_fixture(name):
    """loss, predictions at the label rows, the body's and the fusion's outputs, and the gradients the fixture stores (context
    projection, context table, masked-item vector, item table, task projection, last layer) against the reference's own step,
    with the tolerances tests/test_e2e_gpu.py::test_train_step_matches_reference applies to xlnet_clm_item_train, unchanged"""
    import golden_utils as gu
    import test_e2e_gpu as e2e

    mode = FIXTURES[name]
    d = gu.load(name)
    model = _fixture_model(d).train()
    fusion = model.heads[0].body
    x = {k[3:]: gu.t(v).to(DEV) for k, v in d.items() if k.startswith("in/")}
    cap = {}
    hooks = [model.transformer_block.register_forward_hook(lambda m, i, o: cap.__setitem__("hidden", o.detach().clone())),
             fusion.post_context_module.register_forward_hook(lambda m, i, o: cap.__setitem__("context", o.detach().clone())),
             fusion.register_forward_hook(lambda m, i, o: cap.__setitem__("fused", o.detach().clone()))]
    out = model(x, training=True)
    for h in hooks:
        h.remove()
    masking = model.input_features.masking
    assert torch.equal(masking.mask_schema.cpu(), gu.t(d["out/mask_schema"]))
    assert torch.equal(masking.masked_targets.cpu(), gu.t(d["out/masked_targets"]))
    assert torch.equal(out["labels"].cpu(), gu.t(d["out/labels"]))
    grad_tol = dict(rtol=2e-4, atol=1e-4)
    for what in ("hidden", "context", "fused"):
        _note(f"fixture/{mode}/{what}", _tol_ratio(cap[what], gu.t(d["out/" + what]), e2e.TOL))
        e2e.close(cap[what], gu.t(d["out/" + what]))
    _note(f"fixture/{mode}/predictions", _tol_ratio(out["predictions"], gu.t(d["out/predictions"]), e2e.TOL))
    _note(f"fixture/{mode}/loss", _tol_ratio(out["loss"], gu.t(d["out/loss"]), e2e.TOL))
    e2e.close(out["predictions"], gu.t(d["out/predictions"]))
    e2e.close(out["loss"], gu.t(d["out/loss"]))
    assert abs(float(out["loss"]) - float(d["out/loss"])) < 1e-3
    assert float((out["predictions"].cpu() - gu.t(d["out/predictions"])).abs().max()) < 1e-3
    out["loss"].backward()
    g = gu.section(d, "g/")
    named = dict(model.named_parameters())
    need = [BODY + "post_context_module.embedding_tables.category.weight", BODY + "sequential_module.0._masking.masked_item_embedding",
            BODY + "sequential_module.1.transformer.layer.1.rel_attn.q", BODY + "sequential_module.1.transformer.layer.1.ff.layer_1.weight"]
    need += ["heads.0.prediction_task_dict.next-item.task_block.0.0.weight"] if mode == "concat" else \
        [BODY + "context_projection.weight", BODY + "context_projection.bias"]
    assert set(need) <= set(g), sorted(set(need) - set(g))
    for k, ref in g.items():
        assert k in named and named[k].grad is not None, k
        short = k.replace(BODY, "").replace("sequential_module.", "").replace("heads.0.prediction_task_dict.", "")
        r = _tol_ratio(named[k].grad, ref, grad_tol)
        _note(f"fixture/{mode}/g/{short}", r)
        print(f"{name} {short}: {r:.3f}")
        e2e.close(named[k].grad, ref, msg=lambda m, k=k: f"{k}: {m}", **grad_tol)
    assert len(g) >= 20


@pytest.mark.parametrize("context", ["session", "sequence"])
@pytest.mark.parametrize("aggregation", AGGREGATIONS)
def test_model_with_fusion_trains_and_equals_the_restated_fusion_of_its_parts(aggregation, context):
    mode = MODE_OF[aggregation]
    model = _model(aggregation, context).train()
    fusion = model.heads[0].body
    x = _batch(context)
    seen = {}

    def keep(_mod, _inp, out):
        out.register_hook(lambda g: seen.__setitem__("dout", g.detach().clone()))
        seen["out"] = out.detach().clone()

    hooks = [fusion.register_forward_hook(keep),
             fusion.sequential_module.register_forward_hook(lambda _m, _i, out: seen.__setitem__("seq", out.detach().clone())),
             fusion.post_context_module.register_forward_hook(lambda _m, _i, out: seen.__setitem__("ctx", out.detach().clone()))]
    out = model(x, training=True)
    assert bool(torch.isfinite(out["loss"]))
    out["loss"].backward()
    for h in hooks:
        h.remove()
    assert seen["ctx"].shape == ((B, 24) if context == "session" else (B, L, 24))
    assert seen["out"].shape == (B, L, fusion.last_dim)
    lin = getattr(fusion, "context_projection", None)
    W = lin.weight.detach().cpu() if lin is not None else torch.zeros(D, 24)
    b = lin.bias.detach().cpu() if lin is not None else torch.zeros(D)
    seq, ctx, dout = seen["seq"].cpu(), seen["ctx"].cpu(), seen["dout"].cpu()
    want, bound = R.forward(seq, ctx, W, b, mode)
    r = R.ratio(seen["out"].cpu(), want, bound)
    _note(f"model/out/{mode}", r)
    assert r <= 1.0
    ref = R.gradients(dout, seq, ctx, W, b, mode)
    if lin is not None:
        for name, p in (("d_w", lin.weight), ("d_b", lin.bias)):
            r = R.ratio(p.grad.cpu(), *ref[name])
            _note(f"model/{name}/{mode}", r)
            assert r <= 1.0, name
    # the context table: the rows of d ctx scattered by id; n terms per row, each within its own bound
    tab = _context_table(model, context)
    ids = x["user" if context == "session" else "category"].reshape(-1).cpu()
    dctx, dbound = ref["dctx"]
    cols = slice(16, 24) if context == "session" else slice(0, 24)            # sorted names: country | user
    dctx, dbound = dctx.reshape(ids.numel(), 24)[:, cols], (dbound if dbound is not None else torch.zeros_like(dctx)).reshape(ids.numel(), 24)[:, cols]
    keep_rows = torch.ones_like(ids, dtype=torch.bool) if context == "session" else ids != 0       # the padding id gets no gradient
    want_tab = torch.zeros(tab.shape, dtype=torch.float64).index_add_(0, ids[keep_rows], dctx[keep_rows])
    n = ids.numel()
    tab_bound = torch.zeros(tab.shape, dtype=torch.float64).index_add_(0, ids[keep_rows], (dbound + (n + 3) * R.EPS * dctx.abs())[keep_rows])
    r = R.ratio(tab.grad.cpu(), want_tab, tab_bound)
    _note(f"model/context_table/{mode}/{context}", r)
    assert r <= 1.0 and float(tab.grad.abs().max()) > 0
    assert model.input_features.masking.masked_item_embedding.grad is not None
    from transformers4rec_amd.model import last_rows_gate
    assert last_rows_gate(model, True, B, L) is None


@pytest.mark.parametrize("context", ["session", "sequence", "tabular"])
@pytest.mark.parametrize("aggregation", AGGREGATIONS)
def test_fast_path_and_autograd_visible_gradients_are_equal(aggregation, context):
    x = _batch(context)
    grads = {}
    for visible in (False, True):
        model = _model(aggregation, context).train()
        if visible:
            tr.enable_autograd_gradients(model)
        model(x, training=True)["loss"].backward()
        grads[visible] = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    assert set(grads[False]) <= set(grads[True])
    assert any("post_context_module" in k for k in grads[False])
    assert (aggregation == "concat") != any("context_projection" in k for k in grads[False])
    for k in grads[False]:
        assert torch.equal(grads[True][k], grads[False][k]), k
    assert all(float(grads[True][k].abs().max()) == 0.0 for k in set(grads[True]) - set(grads[False]))


@pytest.mark.parametrize("aggregation", ["elementwise-mul", "concat"])
def test_one_fused_adam_step_moves_the_projection_and_the_context_table(aggregation):
    model = _model(aggregation, "session").train()
    x = _batch("session")
    dense, tables = tr.flatten_model(model)
    opt = tr.FusedAdam([b for b in (dense, tables) if b is not None], lr=1e-2)
    named = dict(model.named_parameters())
    keys = ["heads.0.body.post_context_module.embedding_tables.user.weight"]
    if aggregation != "concat":
        keys += ["heads.0.body.context_projection.weight", "heads.0.body.context_projection.bias"]
    assert {id(named[k]) for k in keys} <= {id(p) for p in tr.hip_parameters(model)}
    before = {k: named[k].detach().clone() for k in keys}
    model(x, training=True)["loss"].backward()
    opt.step()
    torch.cuda.synchronize()
    for k in keys:
        moved = (named[k].detach() - before[k]).abs()
        assert float(moved.max()) > 1e-3 and bool(torch.isfinite(named[k]).all()), k      # Adam's first step: lr per element


@pytest.mark.parametrize("context", ["session", "sequence"])
@pytest.mark.parametrize("aggregation", AGGREGATIONS)
def test_evaluation_and_topk_inference_equal_the_restated_fusion(aggregation, context):
    mode = MODE_OF[aggregation]
    model = _model(aggregation, context).eval()
    model.top_k = 5
    fusion = model.heads[0].body
    x = _batch(context)
    with torch.no_grad():
        ev = model(x, testing=True)
        assert bool(torch.isfinite(ev["loss"])) and ev["predictions"].shape[0] == ev["labels"].shape[0]
        seen = {}
        h = fusion.register_forward_hook(lambda _m, _i, out: seen.__setitem__("out", out.detach().clone()))
        scores, items = model(x)
        h.remove()
        assert scores.shape == (B, 5) and items.shape == (B, 5)
        seq = fusion.sequential_module(x, training=False, testing=False)
        ctx = fusion.post_context_module(x, training=False)
    lin = getattr(fusion, "context_projection", None)
    W = lin.weight.detach().cpu() if lin is not None else torch.zeros(D, 24)
    b = lin.bias.detach().cpu() if lin is not None else torch.zeros(D)
    want, bound = R.forward(seq.cpu(), ctx.cpu(), W, b, mode)
    r = R.ratio(seen["out"].cpu(), want, bound)
    _note(f"model/infer/{mode}", r)
    assert r <= 1.0
    assert torch.equal(seen["out"], fusion.fuse(seq, ctx))
