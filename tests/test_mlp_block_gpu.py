"""MLP block on the GPU: the kernels (csrc/mlp_block.hip, include/t4r_hip_mlpblock.h) against float64
(tests/mlp_block_restatement.py) under its per-element bounds, layer by layer on the device's own activations; the exact zero
pattern of the dropout masks; inference = training bits, the scalar path of unaligned operands, bit equality across launch shapes
and runs, accumulation, NULL outputs, red zones around every buffer with an exact workspace; the registered operator; and the
block inside a Model: one training step against the reference's fixtures (tests/golden/mlp_body_*_train.npz,
tools/make_mlp_block_golden.py) at the tolerances of tests/test_e2e_gpu.py, the restated composition in training, evaluation and
inference, both gradient modes, the last-rows path on and off, the fused optimizer, the replay of the masks.

Every numeric test prints the largest observed error / bound ratio; with T4R_RATIO_LOG set to a path the maxima over the run are
also written there as text: profiles/mlp_block_margins.txt is that file."""
import atexit
import os

import pytest
import torch

import mlp_block_restatement as R
import transformers4rec_amd as tr
from abi_arena import FILLS, Arena
from transformers4rec_amd import _lib, ops, torch_ops  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
SEED, OFFSET = 0x5EED1234ABCD, 3

NTOK = [1, 31, 32, 33, 127, 128, 129, 260]           # the edges of a wave's 32 tokens, of 64-token splits, nine workgroups
# (K0, dims, relu, bias, p): odd K, widths across the 32-row tile and the 128-row group, the limits, four layers, N = 1 inside
STACKS = [(1, [1], True, True, 0.3), (3, [33], False, False, 0.3), (48, [96, 64], True, True, 0.0), (48, [96, 64], False, True, 0.3),
          (65, [100, 33, 64], True, False, 0.3), (336, [128], False, True, 0.0), (336, [128], True, False, 0.0),
          (1024, [512, 1, 512, 4], True, True, 0.3)]
RATIOS = {}


def _note(what, ratio):
    RATIOS[what] = max(RATIOS.get(what, 0.0), float(ratio))


MARGINS_HEAD = """MLP block (csrc/mlp_block.hip): worst error / bound per quantity on an MI355X
Written by tests/test_mlp_block_gpu.py:  T4R_RATIO_LOG=profiles/mlp_block_margins.txt pytest -m gpu tests/test_mlp_block_gpu.py
Kernel level (a<i>/, dx/, dW<i>/, db<i>/ by stack): the bounds of tests/mlp_block_restatement.py over the shapes of the test; every
layer's output against the restatement of the device's own a_{i-1}.
model/: the Model with the block against the restated stack of its own inputs-module output, same bounds.
fixture/<name>/<quantity>: the Model with the block against the reference's training step (tests/golden/mlp_body_*_train.npz),
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


def _tag(K0, dims, relu, bias, p):
    return f"{K0}-" + "-".join(map(str, dims)) + ("/relu" if relu else "/lin") + ("/b" if bias else "/nob") + f"/p{p}"


def _dev(k):
    mv = lambda v: None if v is None else v.to(DEV)      # noqa: E731
    return {n: ([mv(t) for t in v] if isinstance(v, list) else mv(v)) for n, v in k.items()}


def _run(k, relu, p, accumulate=False, want_dx=True):
    """training forward and backward of one case through ops -> (acts, dict dx, dW, db), host tensors"""
    d = _dev(k)
    drop = (p, SEED, OFFSET)
    bs = None if all(b is None for b in d["bs"]) else d["bs"]
    acts = ops.mlp_stack_fwd(d["x"], d["Ws"], bs, relu, drop, save_acts=True)
    dW = [g.clone() if accumulate else torch.zeros_like(g) for g in d["dW0"]]
    db = [g.clone() if accumulate else torch.zeros_like(g) for g in d["db0"]]
    dx = ops.mlp_stack_bwd_(d["dout"], d["x"], d["Ws"], acts, relu, drop, dW, db if bs is not None else None, want_dx=want_dx)
    return ([a.cpu() for a in acts],
            dict(dx=None if dx is None else dx.cpu(), dW=[g.cpu() for g in dW], db=[g.cpu() for g in db] if bs is not None else None))


def _check(tag, k, relu, p, acts, grads, accumulate=False):
    T, dims = k["x"].shape[0], [w.shape[0] for w in k["Ws"]]
    keeps = R.keep_masks(SEED, OFFSET, T, dims, p)
    bs = None if all(b is None for b in k["bs"]) else k["bs"]
    worst = {}
    for i, (want, bound) in enumerate(R.forward(k["x"], k["Ws"], bs, relu, p, keeps, acts=acts)):
        worst[f"a{i}"] = r = R.ratio(acts[i], want, bound)
        _note(f"a{i}/{tag}", r)
        assert r <= 1.0, (tag, T, f"a{i}", r)
        if p > 0:       # the zero pattern is the restated mask's: exact zeros where dropped, non-zero where kept and clearly positive
            assert bool((acts[i][~keeps[i]] == 0).all()), (tag, T, i, "a dropped element is not zero")
            clear = keeps[i] & (want.abs() > bound)
            assert bool((acts[i][clear] != 0).all()), (tag, T, i, "a kept element is zero")
    ref = R.backward(k["dout"], k["x"], k["Ws"], bs, acts, relu, p, keeps, k["dW0"] if accumulate else None,
                     k["db0"] if accumulate else None)
    if grads["dx"] is not None:
        worst["dx"] = r = R.ratio(grads["dx"], *ref["dx"])
        _note(f"dx/{tag}", r)
        assert r <= 1.0, (tag, T, "dx", r)
    for i in range(len(dims)):
        for name in ("dW", "db"):
            if grads[name] is None:
                continue
            worst[f"{name}{i}"] = r = R.ratio(grads[name][i], *ref[name][i])
            _note(f"{name}{i}/{tag}", r)
            assert r <= 1.0, (tag, T, name, i, r)
    return worst


# ------------------------------------------------------------------------------------------------ entries against float64
@pytest.mark.parametrize("K0,dims,relu,bias,p", STACKS, ids=[_tag(*s) for s in STACKS])
def test_entries_against_float64(K0, dims, relu, bias, p):
    """training mode at every ntok: every a_i, dx, every d W_i and d b_i within its bound, the masks' zero pattern exact"""
    tag = _tag(K0, dims, relu, bias, p)
    for T in NTOK:
        k = R.make_case(T, K0, dims, bias)
        acts, grads = _run(k, relu, p)
        worst = _check(tag, k, relu, p, acts, grads)
        print(f"{tag} T={T}: " + ", ".join(f"{n} {v:.3f}" for n, v in worst.items()))


def test_planted_faults_exceed_the_bounds_at_the_gpu_shapes():
    """the bounds have teeth at the shapes above: each planted forward fault of the restatement is far outside"""
    k = R.make_case(129, 65, [100, 33, 64], True)
    keeps = R.keep_masks(SEED, OFFSET, 129, [100, 33, 64], 0.3)
    good = R.forward(k["x"], k["Ws"], k["bs"], True, 0.3, keeps)
    for fault in ("no_bias", "no_scale", "last_act_skipped"):
        bad = R.forward(k["x"], k["Ws"], k["bs"], True, 0.3, keeps, fault=fault)
        i = 2 if fault == "last_act_skipped" else 0
        assert R.ratio(bad[i][0].float(), *good[i]) > 100.0, fault


# ------------------------------------------------------------------------------------------------ bit identity and accumulation
@pytest.mark.parametrize("K0,dims,relu,bias", [(48, [96, 64], True, True), (65, [100, 33, 64], False, False), (336, [128], True, True)])
def test_inference_out_is_the_training_modes_last_activation(K0, dims, relu, bias):
    k = _dev(R.make_case(129, K0, dims, bias))
    bs = k["bs"] if bias else None
    acts = ops.mlp_stack_fwd(k["x"], k["Ws"], bs, relu, (0.0, 0, 0), save_acts=True)
    out = ops.mlp_stack_fwd(k["x"], k["Ws"], bs, relu, (0.0, 0, 0))
    assert out.shape == (129, dims[-1]) and torch.equal(out, acts[-1])
    drop = (0.3, SEED, OFFSET)                    # and with dropout: the same function of (seed, offset)
    assert torch.equal(ops.mlp_stack_fwd(k["x"], k["Ws"], bs, relu, drop), ops.mlp_stack_fwd(k["x"], k["Ws"], bs, relu, drop, save_acts=True)[-1])


@pytest.mark.parametrize("relu", [True, False])
def test_a_row_has_the_same_bits_alone_and_in_a_batch(relu):
    """p = 0 (the mask of a row depends on its index by definition): a row's activations and its dx, alone and at rows 0, 77, 259"""
    K0, dims = 65, [100, 33, 64]
    k = _dev(R.make_case(260, K0, dims, True))
    acts = ops.mlp_stack_fwd(k["x"], k["Ws"], k["bs"], relu, save_acts=True)
    dx = ops.mlp_stack_bwd_(k["dout"], k["x"], k["Ws"], acts, relu)
    for t in (0, 77, 259):
        x1, dout1 = k["x"][t:t + 1].contiguous(), k["dout"][t:t + 1].contiguous()
        one = ops.mlp_stack_fwd(x1, k["Ws"], k["bs"], relu, save_acts=True)
        for a1, a in zip(one, acts):
            assert torch.equal(a1[0], a[t])
        assert torch.equal(ops.mlp_stack_bwd_(dout1, x1, k["Ws"], one, relu)[0], dx[t])
        sub = ops.mlp_stack_fwd(k["x"][t - t % 7:t + 1].contiguous(), k["Ws"], k["bs"], relu)      # another place in the launch
        assert torch.equal(sub[-1], acts[-1][t])


@pytest.mark.parametrize("which", ["x", "W0", "W1", "b0", "dout"])
def test_a_view_at_a_4_byte_offset_takes_the_scalar_path_with_the_same_bits(which):
    k = _dev(R.make_case(129, 48, [96, 64], True))
    drop = (0.3, SEED, OFFSET)

    def run(kk):
        acts = ops.mlp_stack_fwd(kk["x"], kk["Ws"], kk["bs"], True, drop, save_acts=True)
        dW, db = [torch.zeros_like(w) for w in k["Ws"]], [torch.zeros_like(b) for b in k["bs"]]
        dx = ops.mlp_stack_bwd_(kk["dout"], kk["x"], kk["Ws"], acts, True, drop, dW, db)
        return acts + [dx] + dW + db

    def shift(t):
        flat = torch.empty(t.numel() + 1, device=DEV)
        view = flat[1:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view

    shifted = dict(k, Ws=list(k["Ws"]), bs=list(k["bs"]))
    if which in ("x", "dout"):
        shifted[which] = shift(k[which])
    else:
        lst = shifted["Ws" if which[0] == "W" else "bs"]
        lst[int(which[1])] = shift(lst[int(which[1])])
    for a, b in zip(run(k), run(shifted)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("relu,bias,p", [(True, True, 0.3), (False, False, 0.3), (True, True, 0.0)])
def test_two_runs_give_the_same_bits_and_gradients_accumulate(relu, bias, p):
    k = R.make_case(260, 65, [100, 33, 64], bias, seed=1)
    a1, g1 = _run(k, relu, p)
    a2, g2 = _run(k, relu, p)
    for x, y in zip(a1, a2):
        assert torch.equal(x, y)
    assert torch.equal(g1["dx"], g2["dx"])
    names = ("dW", "db") if bias else ("dW",)
    for name in names:
        for x, y in zip(g1[name], g2[name]):
            assert torch.equal(x, y), name
    # accumulated: the batch sum is formed first, then added once to what the buffers held
    acts, g3 = _run(k, relu, p, accumulate=True)
    for i in range(3):
        assert torch.equal(g3["dW"][i], k["dW0"][i] + g1["dW"][i])
        if bias:
            assert torch.equal(g3["db"][i], k["db0"][i] + g1["db"][i])
    assert torch.equal(g3["dx"], g1["dx"])                                   # overwritten, not accumulated
    _check("accumulate", k, relu, p, acts, g3, accumulate=True)
    # a second backward into the same buffers doubles them within one rounding
    d = _dev(k)
    drop = (p, SEED, OFFSET)
    dacts = ops.mlp_stack_fwd(d["x"], d["Ws"], d["bs"] if bias else None, relu, drop, save_acts=True)
    dW = [torch.zeros_like(w) for w in d["Ws"]]
    for _ in range(2):
        ops.mlp_stack_bwd_(d["dout"], d["x"], d["Ws"], dacts, relu, drop, dW, None, want_dx=False)
    for i in range(3):
        assert torch.equal(dW[i].cpu(), g1["dW"][i] + g1["dW"][i])           # x + x is exact


def test_null_outputs_and_no_tokens():
    k = _dev(R.make_case(33, 48, [96, 64], True))
    drop = (0.3, SEED, OFFSET)
    acts = ops.mlp_stack_fwd(k["x"], k["Ws"], k["bs"], True, drop, save_acts=True)
    full_W, full_b = [torch.zeros_like(w) for w in k["Ws"]], [torch.zeros_like(b) for b in k["bs"]]
    dx = ops.mlp_stack_bwd_(k["dout"], k["x"], k["Ws"], acts, True, drop, full_W, full_b)
    only_dx = ops.mlp_stack_bwd_(k["dout"], None, k["Ws"], acts, True, drop)
    assert torch.equal(only_dx, dx)
    w1 = torch.zeros_like(k["Ws"][1])
    assert ops.mlp_stack_bwd_(k["dout"], None, k["Ws"], acts, True, drop, [None, w1], None, want_dx=False) is None
    assert torch.equal(w1, full_W[1])
    b0 = torch.zeros_like(k["bs"][0])
    assert ops.mlp_stack_bwd_(k["dout"], k["x"], k["Ws"], acts, True, drop, None, [b0, None], want_dx=False) is None
    assert torch.equal(b0, full_b[0])
    assert ops.mlp_stack_bwd_(k["dout"], None, k["Ws"], acts, True, drop, want_dx=False) is None       # nothing asked: nothing launches
    empty = ops.mlp_stack_fwd(k["x"][:0], k["Ws"], k["bs"])
    assert empty.shape == (0, 64)
    assert ops.mlp_stack_bwd_(k["dout"][:0], k["x"][:0], k["Ws"], [a[:0] for a in acts]).shape == (0, 48)
    three = ops.mlp_stack_fwd(k["x"].view(3, 11, 48), k["Ws"], k["bs"], True, drop)                   # leading dimensions are kept
    assert three.shape == (3, 11, 64) and torch.equal(three.view(33, 64), acts[-1])


# ------------------------------------------------------------------------------------------------ buffer discipline
@pytest.mark.parametrize("fill", FILLS, ids=["zeros", "ones"])
@pytest.mark.parametrize("relu,bias,p", [(True, True, 0.3), (False, False, 0.3)])
@pytest.mark.parametrize("T,K0,dims", [(65, 65, [100, 33]), (260, 48, [96, 64])])
def test_red_zones_around_every_buffer(T, K0, dims, relu, bias, p, fill):
    """guards around every buffer, the workspace exactly as large as the size query says, under both fills, each call twice"""
    lib = _lib.load()
    k = R.make_case(T, K0, dims, bias)
    n = len(dims)
    Ks = [K0] + dims[:-1]
    Np, keepN = _lib.int_array(dims)
    assert lib.t4r_mlp_stack_supported(n, K0, Np) == 1
    a = Arena(fill, DEV, capacity=16 << 20)
    x = a.new("x", "in", F32, T * K0).set(k["x"])
    Wb = [a.new(f"W{i}", "in", F32, dims[i] * Ks[i]).set(k["Ws"][i]) for i in range(n)]
    bb = [a.new(f"b{i}", "in", F32, dims[i]).set(k["bs"][i]) for i in range(n)] if bias else None
    out = a.new("out", "out", F32, T * dims[-1])
    a.seal()
    Wp, keepW = _lib.ptr_array([w.ptr for w in Wb])
    Bp, keepB = _lib.ptr_array([b.ptr for b in bb]) if bias else (None, None)
    d = _dev(k)
    want = ops.mlp_stack_fwd(d["x"], d["Ws"], d["bs"] if bias else None, relu, (p, SEED, OFFSET), save_acts=True)
    for _ in range(2):              # inference: out only
        rc = lib.t4r_mlp_stack_fwd(_stream(), x.ptr, Wp, Bp, None, out.ptr, T, n, K0, Np, int(relu), p, SEED, OFFSET)
        assert rc == 0, lib.t4r_last_error()
        torch.cuda.synchronize()
        v = a.check()
        assert v is None, str(v)
        assert a.nonfinite() is None
        assert torch.equal(out.t.view(T, dims[-1]), want[-1])
    acts = [a.new(f"a{i}", "out", F32, T * dims[i]) for i in range(n)]
    a.seal()
    Ap, keepA = _lib.ptr_array([t.ptr for t in acts])
    for _ in range(2):              # training: every a_i
        rc = lib.t4r_mlp_stack_fwd(_stream(), x.ptr, Wp, Bp, Ap, None, T, n, K0, Np, int(relu), p, SEED, OFFSET)
        assert rc == 0, lib.t4r_last_error()
        torch.cuda.synchronize()
        v = a.check()
        assert v is None, str(v)
        assert a.nonfinite() is None
        for i in range(n):
            assert torch.equal(acts[i].t.view(T, dims[i]), want[i])
    # ---- backward: the exact workspace
    dyb = a.new("dout", "in", F32, T * dims[-1]).set(k["dout"])
    dx = a.new("dx", "out", F32, T * K0)
    dW = [a.new(f"dW{i}", "inout", F32, dims[i] * Ks[i]).set(0) for i in range(n)]
    db = [a.new(f"db{i}", "inout", F32, dims[i]).set(0) for i in range(n)] if bias else None
    n_ws = lib.t4r_mlp_stack_bwd_ws_floats(T, n, K0, Np)
    assert n_ws > 0
    ws = a.ws("ws", 4 * n_ws)
    a.seal()
    Gp, keepG = _lib.ptr_array([t.ptr for t in dW])
    Hp, keepH = _lib.ptr_array([t.ptr for t in db]) if bias else (None, None)
    first = None
    for _ in range(2):
        for t in dW + (db or []):
            t.t.zero_()
        rc = lib.t4r_mlp_stack_bwd(_stream(), dyb.ptr, x.ptr, Wp, Ap, dx.ptr, Gp, Hp, ws.ptr, T, n, K0, Np, int(relu), p, SEED, OFFSET)
        assert rc == 0, lib.t4r_last_error()
        torch.cuda.synchronize()
        v = a.check()
        assert v is None, str(v)
        assert a.nonfinite() is None
        got = [dx.bits()] + [t.bits() for t in dW + (db or [])]
        if first is None:
            first = got
        for p0, p1 in zip(first, got):
            assert torch.equal(p0, p1)
    grads = dict(dx=dx.t.view(T, K0).cpu(), dW=[dW[i].t.view(dims[i], Ks[i]).cpu() for i in range(n)],
                 db=[t.t.cpu() for t in db] if bias else None)
    _check("arena", k, relu, p, [acts[i].t.view(T, dims[i]).cpu() for i in range(n)], grads)


# ------------------------------------------------------------------------------------------------ registered operator
@pytest.mark.parametrize("relu,bias,p", [(True, True, 0.3), (False, False, 0.0)])
def test_registered_operator_equals_the_ctypes_call_and_differentiates(relu, bias, p):
    k = _dev(R.make_case(33, 48, [96, 64], bias))
    x = k["x"].clone().requires_grad_()
    Ws = [w.clone().requires_grad_() for w in k["Ws"]]
    bs = [b.clone().requires_grad_() for b in k["bs"]] if bias else []
    out = torch.ops.t4r_hip.mlp_stack(x, Ws, bs, relu, p, SEED, OFFSET)
    acts = ops.mlp_stack_fwd(k["x"], k["Ws"], k["bs"] if bias else None, relu, (p, SEED, OFFSET), save_acts=True)
    assert torch.equal(out, acts[-1])
    out.backward(k["dout"])
    dW, db = [torch.zeros_like(w) for w in k["Ws"]], [torch.zeros_like(w[:, 0]) for w in k["Ws"]]
    dx = ops.mlp_stack_bwd_(k["dout"], k["x"], k["Ws"], acts, relu, (p, SEED, OFFSET), dW, db if bias else None)
    assert torch.equal(x.grad, dx)
    for i in range(2):
        assert torch.equal(Ws[i].grad, dW[i])
        if bias:
            assert torch.equal(bs[i].grad, db[i])


# ------------------------------------------------------------------------------------------------ module level
V, L, D_ITEM, D, B = 50, 20, 48, 64, 13


def _model(dims=(96, 64), masking="clm", arch="xlnet", seed=0, **mlp_kw):
    """items 48 wide, the block, XLNet (or GPT-2) d 64, 2 layers, 4 heads, L 20, tied head"""
    torch.manual_seed(seed)
    feats = tr.TabularSequenceFeatures.from_schema(tr.session_schema(V, L), max_sequence_length=L, masking=masking,
                                                   aggregation="concat", embedding_dims={"item_id": D_ITEM})
    if arch == "xlnet":
        cfg = tr.XLNetConfig.build(d_model=D, n_head=4, n_layer=2, total_seq_length=L, dropout=0.0)
    else:
        cfg = tr.GPT2Config.build(d_model=D, n_head=4, n_layer=2, total_seq_length=L, dropout=0.0)
    model = tr.Model(feats, tr.TransformerBlock(cfg, masking=feats.masking), tr.NextItemPredictionTask(weight_tying=True),
                     mlp_block=tr.MLPBlock(list(dims), **mlp_kw))
    return model.to(DEV)


def _batch(n=B):
    g = torch.Generator().manual_seed(5)
    lens = torch.randint(5, L + 1, (n,), generator=g)
    lens[0] = L
    m = torch.arange(L)[None] < lens[:, None]
    return {"item_id": (torch.randint(1, V + 1, (n, L), generator=g) * m).to(DEV)}


def _watch(model, seen, with_grad=True):
    stack = model.mlp_block

    def keep(_mod, _inp, out):
        if with_grad and out.requires_grad:
            out.register_hook(lambda g: seen.__setitem__("dout", g.detach().clone()))
        seen["out"] = out.detach().clone()

    return [stack.register_forward_hook(keep),
            model.input_features.register_forward_hook(lambda _m, _i, out: seen.__setitem__("x", out.detach().clone()))]


def _check_stack_output(tag, stack, seen, drop):
    """the block's output is the ops call's bits on the input block's output, and every layer is within its bound of the restated
    layer on the device's own a_{i-1}; -> (device acts, keeps) on the host"""
    x = seen["x"]
    Ws, bs = stack._weights(), stack._biases()
    acts = ops.mlp_stack_fwd(x.contiguous(), Ws, bs, stack.relu, drop, save_acts=True)
    assert torch.equal(acts[-1], seen["out"])
    T = x.numel() // x.shape[-1]
    dims = [w.shape[0] for w in Ws]
    keeps = R.keep_masks(drop[1], drop[2], T, dims, drop[0])
    host = [a.cpu().view(T, -1) for a in acts]
    ref = R.forward(x.cpu().view(T, -1), [w.cpu() for w in Ws], None if bs is None else [b.cpu() for b in bs], stack.relu, drop[0],
                    keeps, acts=host)
    for i, (want, bound) in enumerate(ref):
        r = R.ratio(host[i], want, bound)
        _note(f"model/{tag}/a{i}", r)
        assert r <= 1.0, (tag, i, r)
        if drop[0] > 0:
            assert bool((host[i][~keeps[i]] == 0).all())
    return host, keeps


def _check_stack_grads(tag, stack, seen, drop, host, keeps):
    Ws, bs = stack._weights(), stack._biases()
    T = host[0].shape[0]
    ref = R.backward(seen["dout"].cpu().view(T, -1), seen["x"].cpu().view(T, -1), [w.cpu() for w in Ws],
                     None if bs is None else [b.cpu() for b in bs], host, stack.relu, drop[0], keeps)
    for i, dense in enumerate(stack):
        r = R.ratio(dense[0].weight.grad.cpu(), *ref["dW"][i])
        _note(f"model/{tag}/dW{i}", r)
        assert r <= 1.0 and float(dense[0].weight.grad.abs().max()) > 0, (tag, "dW", i, r)
        if bs is not None:
            r = R.ratio(dense[0].bias.grad.cpu(), *ref["db"][i])
            _note(f"model/{tag}/db{i}", r)
            assert r <= 1.0, (tag, "db", i, r)


# ------------------------------------------------------------------------------------------------ against the reference's step
FIXTURES = ("mlp_body_clm_train", "mlp_body_linear_clm_train")


def _fixture_model(d):
    """the mirror of tools/make_mlp_block_golden.py's reference model, with the reference's parameters"""
    import test_e2e_gpu as e2e

    Lf, Vf = int(d["meta/L"]), int(d["meta/V"])
    feats = tr.TabularSequenceFeatures.from_schema(tr.session_schema(Vf - 1, Lf), max_sequence_length=Lf, masking="clm",
                                                   aggregation="concat", embedding_dims={"item_id": int(d["meta/d_item"])})
    cfg = tr.XLNetConfig.build(d_model=int(d["meta/d_model"]), n_head=int(d["meta/n_head"]), n_layer=int(d["meta/n_layer"]),
                               total_seq_length=Lf, dropout=0.0)
    mlp = tr.MLPBlock([int(v) for v in str(d["meta/dimensions"]).split(",")],
                      activation=torch.nn.ReLU if int(d["meta/relu"]) else None, use_bias=bool(int(d["meta/use_bias"])))
    model = tr.Model(feats, tr.TransformerBlock(cfg, masking=feats.masking), tr.NextItemPredictionTask(weight_tying=True), mlp_block=mlp)
    e2e.load_reference_state(model, d)
    return model.to(DEV)


def _tol_ratio(got, want, tol):
    got, want = got.detach().cpu().double(), want.double()
    return float(((got - want).abs() / (tol["atol"] + tol["rtol"] * want.abs())).max())


@pytest.mark.parametrize("name", FIXTURES)
def test_train_step_matches_the_reference_fixture(name):
    """the block's output, the hidden states, loss, labels, predictions and the gradients the fixture stores (the stack, the
    masked-item vector, the item table, the task projection, the last layer) against the reference's own step, with the
    tolerances tests/test_e2e_gpu.py::test_train_step_matches_reference applies to xlnet_clm_item_train, unchanged"""
    import golden_utils as gu
    import test_e2e_gpu as e2e

    d = gu.load(name)
    model = _fixture_model(d).train()
    x = {k[3:]: gu.t(v).to(DEV) for k, v in d.items() if k.startswith("in/")}
    cap = {}
    hooks = [model.transformer_block.register_forward_hook(lambda m, i, o: cap.__setitem__("hidden", o.detach().clone())),
             model.mlp_block.register_forward_hook(lambda m, i, o: cap.__setitem__("mlp", o.detach().clone()))]
    out = model(x, training=True)
    for h in hooks:
        h.remove()
    masking = model.input_features.masking
    assert torch.equal(masking.mask_schema.cpu(), gu.t(d["out/mask_schema"]))
    assert torch.equal(masking.masked_targets.cpu(), gu.t(d["out/masked_targets"]))
    assert torch.equal(out["labels"].cpu(), gu.t(d["out/labels"]))
    grad_tol = dict(rtol=2e-4, atol=1e-4)
    for what in ("mlp", "hidden"):
        _note(f"fixture/{name}/{what}", _tol_ratio(cap[what], gu.t(d["out/" + what]), e2e.TOL))
        e2e.close(cap[what], gu.t(d["out/" + what]))
    _note(f"fixture/{name}/predictions", _tol_ratio(out["predictions"], gu.t(d["out/predictions"]), e2e.TOL))
    _note(f"fixture/{name}/loss", _tol_ratio(out["loss"], gu.t(d["out/loss"]), e2e.TOL))
    e2e.close(out["predictions"], gu.t(d["out/predictions"]))
    e2e.close(out["loss"], gu.t(d["out/loss"]))
    assert abs(float(out["loss"]) - float(d["out/loss"])) < 1e-3
    assert float((out["predictions"].cpu() - gu.t(d["out/predictions"])).abs().max()) < 1e-3
    out["loss"].backward()
    g = gu.section(d, "g/")
    named = dict(model.named_parameters())
    need = ["heads.0.body.1.0.0.weight", "heads.0.body.0._masking.masked_item_embedding",
            "heads.0.body.0.to_merge.categorical_module.embedding_tables.item_id.weight",
            "heads.0.body.2.transformer.layer.1.rel_attn.q", "heads.0.prediction_task_dict.next-item.task_block.0.0.weight"]
    assert set(need) <= set(g), sorted(set(need) - set(g))
    for k, ref in g.items():
        assert k in named and named[k].grad is not None, k
        short = k.replace("heads.0.body.", "").replace("heads.0.prediction_task_dict.", "")
        r = _tol_ratio(named[k].grad, ref, grad_tol)
        _note(f"fixture/{name}/g/{short}", r)
        print(f"{name} {short}: {r:.3f}")
        e2e.close(named[k].grad, ref, msg=lambda m, k=k: f"{k}: {m}", **grad_tol)
    assert len(g) >= 20


# ------------------------------------------------------------------------------------------------ own checks
@pytest.mark.parametrize("arch,kw", [("xlnet", dict(dims=(96, 64), dropout=0.3)), ("xlnet", dict(dims=(64,), activation=None, use_bias=False, dropout=0.3)),
                                     ("gpt2", dict(dims=(96, 64), dropout=0.3))], ids=["xlnet-relu", "xlnet-linear", "gpt2-relu"])
def test_a_training_step_equals_the_restated_stack_of_its_inputs(arch, kw):
    """dropout 0.3 in the block, XLNet and GPT-2 bodies: the input block's output through the restated stack (float64, the device's
    masks) at the block's output, the stack's gradients from the gradient that arrives there; the loss is finite"""
    model = _model(arch=arch, **kw).train()
    stack = model.mlp_block
    seen = {}
    hooks = _watch(model, seen)
    out = model(_batch(), training=True)
    assert bool(torch.isfinite(out["loss"])) and stack._drop_offset == 1
    out["loss"].backward()
    for h in hooks:
        h.remove()
    assert seen["x"].shape == (B, L, D_ITEM) and seen["out"].shape == (B, L, D)
    drop = (0.3, stack.seed, 1)
    tag = arch + ("/relu" if stack.relu else "/linear")
    host, keeps = _check_stack_output(tag, stack, seen, drop)
    _check_stack_grads(tag, stack, seen, drop, host, keeps)
    memb = model.input_features.masking.masked_item_embedding
    assert memb.shape == (D_ITEM,) and memb.grad is not None
    assert float(model.input_features.item_embedding_table.weight.grad.abs().max()) > 0


def test_fast_path_and_autograd_visible_gradients_are_equal():
    x = _batch()
    grads = {}
    for visible in (False, True):
        model = _model(dropout=0.3).train()
        if visible:
            tr.enable_autograd_gradients(model)
        model(x, training=True)["loss"].backward()
        grads[visible] = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    assert set(grads[False]) <= set(grads[True])
    assert {f"heads.0.body.1.{i}.0.{n}" for i in (0, 1) for n in ("weight", "bias")} <= set(grads[False])
    for k in grads[False]:
        assert torch.equal(grads[True][k], grads[False][k]), k
    assert all(float(grads[True][k].abs().max()) == 0.0 for k in set(grads[True]) - set(grads[False]))


def test_gradients_with_the_last_rows_path_on_equal_those_with_it_off():
    """MLM with the tied head: the three-entry body keeps the last-rows path; same loss, labels and predictions, the
    gradients within the tolerance tests/test_last_rows_gpu.py::test_model_step_last_rows_on_and_off applies"""
    from test_last_rows_gpu import GRAD_TOL, close
    from transformers4rec_amd import transformer as tfm

    x = _batch(64)
    res = {}
    for on in (True, False):
        model = _model(dims=(96, 64), masking="mlm").train()
        prev = tfm._LAST_ROWS
        tfm._LAST_ROWS = on
        try:
            out = model(x, training=True)
            ran = model.transformer_block.transformer.last_out_rows
            out["loss"].backward()
            torch.cuda.synchronize()
        finally:
            tfm._LAST_ROWS = prev
        preds = out["predictions"]
        preds = preds.materialize() if hasattr(preds, "materialize") else preds
        res[on] = (out["loss"].detach().clone(), out["labels"].clone(), preds.detach().clone(),
                   {k: q.grad.detach().clone() for k, q in model.named_parameters() if q.grad is not None}, ran)
    assert res[False][4] is None and res[True][4] is not None and 0 < res[True][4] <= 64 * L // 2
    for i in range(3):
        assert torch.equal(res[True][i], res[False][i])
    g1, g0 = res[True][3], res[False][3]
    assert set(g1) == set(g0) and "heads.0.body.1.0.0.weight" in g1
    for k in g0:
        close(g1[k].reshape(-1), g0[k].reshape(-1), rtol=2 * GRAD_TOL[0], atol=2 * GRAD_TOL[1], msg=lambda mm, k=k: f"{k}: {mm}")


def test_one_fused_adam_step_moves_every_stack_parameter():
    model = _model(dropout=0.1).train()
    dense, tables = tr.flatten_model(model)
    opt = tr.FusedAdam([b for b in (dense, tables) if b is not None], lr=1e-2)
    named = dict(model.named_parameters())
    keys = [f"heads.0.body.1.{i}.0.{n}" for i in (0, 1) for n in ("weight", "bias")]
    assert {id(named[k]) for k in keys} <= {id(p) for p in tr.hip_parameters(model)}
    before = {k: named[k].detach().clone() for k in keys}
    model(_batch(), training=True)["loss"].backward()
    opt.step()
    torch.cuda.synchronize()
    for k in keys:
        moved = (named[k].detach() - before[k]).abs()
        assert float(moved.max()) > 1e-3 and bool(torch.isfinite(named[k]).all()), k      # Adam's first step: lr per element


def test_rng_state_replays_the_blocks_masks():
    model = _model(dropout=0.3).train()
    x = _batch()
    seen = {}
    hooks = _watch(model, seen, with_grad=False)
    with torch.no_grad():
        model(x, training=True)
        state = tr.get_rng_state(model)
        assert state["heads.0.body.1"]["_drop_offset"] == 1
        model(x, training=True)
        second = seen["out"].clone()
        model(x, training=True)
        third = seen["out"].clone()
        tr.set_rng_state(model, state)
        model(x, training=True)
    for h in hooks:
        h.remove()
    assert torch.equal(seen["out"], second) and not torch.equal(second, third)
    assert ((second == 0) != (third == 0)).any()


@pytest.mark.parametrize("masking", ["clm", "mlm"])
def test_evaluation_and_topk_inference_equal_the_restated_composition(masking):
    model = _model(masking=masking, dropout=0.3).eval()
    model.top_k = 5
    stack = model.mlp_block
    x = _batch()
    with torch.no_grad():
        seen = {}
        hooks = _watch(model, seen, with_grad=False)
        ev = model(x, testing=True)
        assert bool(torch.isfinite(ev["loss"])) and ev["predictions"].shape[0] == ev["labels"].shape[0]
        _check_stack_output(f"eval/{masking}", stack, seen, ops.NO_DROP)                 # evaluation: no dropout
        scores, items = model(x)
        for h in hooks:
            h.remove()
        assert scores.shape == (B, 5) and items.shape == (B, 5) and stack._drop_offset == 0
        assert seen["x"].shape == (B, L + 1 if masking == "mlm" else L, D_ITEM)          # MLM inference: one more position
        _check_stack_output(f"infer/{masking}", stack, seen, ops.NO_DROP)
        assert torch.equal(seen["out"], ops.mlp_stack_fwd(seen["x"].contiguous(), stack._weights(), stack._biases(), stack.relu))
