"""The last XLNet layer on the label rows only (include/t4r_hip_rows.h: t4r_xlnet_layer_fwd_rows / _bwd_rows).

Per-row results are the plain entries' bit for bit (a row's arithmetic does not depend on the tile it sits in); the forward
is exactly zero off the map; the backward reads dh_out on the map only; the batch-reduced parameter gradients meet the bounds
tests/test_kernels_gpu.py::test_xlnet_layer_dropout_fwd_bwd applies to the full path against the fp64 restatement, and are
within twice those bounds of the full path (triangle inequality: the differences are summation order only)."""
import numpy as np
import pytest
import torch

import t4r_oracle as O
from test_kernels_gpu import ORDER, _layer_params, _mask, close, cu

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 0.03
SHAPES = [(9, 20, 128, 4), (300, 20, 64, 4), (5, 32, 128, 4), (1, 20, 128, 4)]
DROPS = [0.0, 0.3]
# the bounds of test_xlnet_layer_dropout_fwd_bwd (full path against the oracle)
OUT_ATOL, DH_TOL, GRAD_TOL = 5e-5, (1e-4, 3e-4), (1e-4, 8e-4)


@pytest.fixture(scope="module")
def ops():
    from transformers4rec_amd import ops as _ops

    return _ops


def _row_sets(B, L):
    T = B * L
    g = np.random.default_rng(B * 1000 + L)
    pick = lambda k: np.sort(g.choice(T, k, replace=False))
    sets = {"one": np.array([T // 2]), "ends": np.array([0, T - 1]), "n15": pick(15), "n16": pick(16), "n17": pick(17)}
    if B in (9, 300):
        sets["n81"] = pick(81)
    m = g.random(T) < 0.15
    for b in range(B):          # at least one row per session
        if not m[b * L:(b + 1) * L].any():
            m[b * L + int(g.integers(L))] = True
    sets["bern"] = np.nonzero(m)[0]
    sets["all"] = np.arange(T)
    return sets


CASES = [(s, p, name) for s in SHAPES for p in DROPS for name in _row_sets(s[0], s[1])]
_STATE = {}


def _kw(ops, p):
    # dropout 0.3: the last layer of a stack in training mode (the model-level output dropout rides in the feed-forward kernels)
    return dict(drop_p=p, seed=99, offset=7, layer_idx=2 | (ops.LAYER_FUSE_FINAL if p > 0 else 0))


def _state(ops, shape, p):
    """inputs and the full layer's forward of one (shape, dropout): computed once, shared, never written"""
    key = (shape, p)
    if key not in _STATE:
        B, L, D, n = shape
        g = torch.Generator().manual_seed(B * 3 + D)
        prm = _layer_params(g, D, n)
        h = torch.randn(B, L, D, generator=g)
        dout = torch.randn(B * L, D, generator=g)
        pos = cu(O.xlnet_pos_emb(L, D))
        params = [cu(prm[k]) for k in ORDER]
        h2 = cu(h).view(B * L, D)
        out, ws = ops.xlnet_layer_fwd(h2, pos, params, B, L, n, EPS, **_kw(ops, p))
        _STATE[key] = dict(prm=prm, h=h, h2=h2, dout=cu(dout), pos=pos, params=params, out=out, ws=ws)
    return _STATE[key]


def _fwd_rows_into(ops, st, shape, p, rows, n_rows, out):
    """t4r_xlnet_layer_fwd_rows into a buffer of the caller's (ops.xlnet_layer_fwd allocates its own)"""
    from transformers4rec_amd import _lib

    B, L, D, n = shape
    kw = _kw(ops, p)
    ws = torch.empty(ops.xlnet_layer_ws_floats(B, L, D, n, p > 0), device=DEV, dtype=torch.float32)
    parr, _keep = _lib.ptr_array([t.data_ptr() for t in st["params"]])
    _lib.call("t4r_xlnet_layer_fwd_rows", ops._stream(), st["h2"].data_ptr(), st["pos"].data_ptr(), parr, ws.data_ptr(),
              out.data_ptr(), B, L, D, n, EPS, float(p), kw["seed"], kw["offset"], kw["layer_idx"], None, None,
              rows.data_ptr(), int(n_rows))
    return ws


def _bwd(ops, st, shape, p, ws, dout, rows=None, n_rows=None):
    B, L, D, n = shape
    grads = [torch.zeros_like(t) for t in st["params"]]
    dh = ops.xlnet_layer_bwd(st["h2"], st["pos"], st["params"], grads, ws, dout, B, L, n, EPS, rows=rows, n_rows=n_rows,
                             **_kw(ops, p))
    return dh, grads


@pytest.mark.parametrize("shape,p,name", CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}-p{p}-{nm}" for s, p, nm in CASES])
def test_layer_rows_bitwise_and_confined(ops, shape, p, name):
    B, L, D, n = shape
    T = B * L
    st = _state(ops, shape, p)
    idx = torch.from_numpy(_row_sets(B, L)[name]).to(DEV)
    nr = int(idx.numel())
    rows = torch.full((T,), -1, device=DEV, dtype=torch.int32)       # the label compaction's layout: first n entries valid
    rows[:nr] = idx.to(torch.int32)
    off = torch.ones(T, dtype=torch.bool, device=DEV)
    off[idx] = False
    # ---- forward: the mapped rows bit for bit, exact zeros elsewhere even in a NaN-filled buffer
    out = torch.full((T, D), float("nan"), device=DEV)
    ws = _fwd_rows_into(ops, st, shape, p, rows, nr, out)
    assert torch.equal(out[idx], st["out"][idx])
    assert not bool(out[off].ne(0).any()) and not bool(torch.isnan(out).any())
    # ---- backward: a gradient that is zero off the map -> d h of the full layer bit for bit
    dout0 = st["dout"].clone()
    dout0[off] = 0
    dh_full, g_full = _bwd(ops, st, shape, p, st["ws"], dout0)
    dh, g = _bwd(ops, st, shape, p, ws, dout0, rows, nr)
    assert torch.equal(dh, dh_full), f"max |d| {float((dh - dh_full).abs().max()):.3e}"
    # ---- the map confines the reads: NaN off the map changes nothing (and a second run gives the same bits)
    doutn = st["dout"].clone()
    doutn[off] = float("nan")
    dh_n, g_n = _bwd(ops, st, shape, p, ws, doutn, rows, nr)
    assert torch.equal(dh_n, dh)
    for k, a, b in zip(ORDER, g_n, g):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), k
    # ---- parameter gradients: within twice the layer bound of the full path (summation order only)
    for k, a, b in zip(ORDER, g, g_full):
        close(a.reshape(-1), b.reshape(-1), rtol=2 * GRAD_TOL[0], atol=2 * GRAD_TOL[1], msg=lambda mm, k=k: f"{k}: {mm}")
    if name == "all":       # every row mapped: also the plain entry's forward as a whole
        assert torch.equal(out, st["out"])


@pytest.mark.parametrize("shape", [(9, 20, 128, 4), (300, 20, 64, 4)], ids=["9x20x128", "300x20x64"])
def test_layer_rows_against_the_fp64_restatement(ops, shape):
    """the mapped path meets the bounds the full path is held to (dropout 0.3, the model-level output dropout fused)"""
    B, L, D, n = shape
    T, p = B * L, 0.3
    st = _state(ops, shape, p)
    kw = _kw(ops, p)
    idx_c = torch.from_numpy(_row_sets(B, L)["bern"])
    idx = idx_c.to(DEV)
    rows = idx.to(torch.int32).contiguous()
    C = lambda site: ops.dropout_ctr_hi(kw["offset"], 2, site)
    masks = dict(pos=_mask(ops, (B, 2 * L, D), p, kw["seed"], ops.dropout_ctr_hi(kw["offset"], 255, ops.SITE_POS)),
                 prob=_mask(ops, (B, n, L, L), p, kw["seed"], C(ops.SITE_PROB)),
                 attn_out=_mask(ops, (B, L, D), p, kw["seed"], C(ops.SITE_ATTN_OUT)),
                 ff_act=_mask(ops, (B, L, 4 * D), p, kw["seed"], C(ops.SITE_FF_ACT)),
                 ff_out=_mask(ops, (B, L, D), p, kw["seed"], C(ops.SITE_FF_OUT)))
    final = _mask(ops, (B, L, D), p, kw["seed"], ops.dropout_ctr_hi(kw["offset"], 255, ops.SITE_FINAL)).double()
    pr = {k: v.double().requires_grad_() for k, v in st["prm"].items()}
    hr = st["h"].double().requires_grad_()
    ref = O.xlnet_layer_dropout(hr, pr, n, EPS, {k: v.double() for k, v in masks.items()}, p) * final / (1 - p)
    dout0 = torch.zeros(T, D, dtype=torch.float64)
    dout0[idx_c] = st["dout"].cpu().double()[idx_c]
    ref.backward(dout0.view(B, L, D))
    out, ws = ops.xlnet_layer_fwd(st["h2"], st["pos"], st["params"], B, L, n, EPS, rows=rows, n_rows=int(idx.numel()), **kw)
    close(out[idx], ref.detach().reshape(T, D)[idx_c].float(), atol=OUT_ATOL)
    dh, g = _bwd(ops, st, shape, p, ws, cu(dout0.float()), rows, int(idx.numel()))
    close(dh, hr.grad.reshape(T, D).float(), rtol=DH_TOL[0], atol=DH_TOL[1])
    for k, gt in zip(ORDER, g):
        close(gt.reshape(-1), pr[k].grad.reshape(-1).float(), rtol=GRAD_TOL[0], atol=GRAD_TOL[1], msg=lambda mm, k=k: f"{k}: {mm}")


def test_layer_rows_refusals(ops):
    """n = 0, n > T, an unsupported width, key_len given: rc != 0 with a message, checked before any launch (the buffers are null)"""
    from transformers4rec_amd import _lib

    lib = _lib.load()
    rows = torch.zeros(64, device=DEV, dtype=torch.int32)
    kl = torch.ones(2, device=DEV, dtype=torch.int32)

    def both(B, L, D, n_head, key_len, n, word):
        for name, lead in (("t4r_xlnet_layer_fwd_rows", (None,) * 6), ("t4r_xlnet_layer_bwd_rows", (None,) * 9)):
            rc = getattr(lib, name)(*lead, B, L, D, n_head, EPS, 0.0, 0, 0, 0, key_len, None, rows.data_ptr(), n)
            assert rc != 0 and word in lib.t4r_last_error(), (name, lib.t4r_last_error())

    both(2, 20, 64, 4, None, 0, b"mapped rows")
    both(2, 20, 64, 4, None, 41, b"mapped rows")
    both(2, 20, 48, 4, None, 5, b"token-tile")
    both(2, 20, 64, 4, kl.data_ptr(), 5, b"key_len")
    rc = lib.t4r_xlnet_layer_fwd_rows(*(None,) * 6, 2, 20, 64, 4, EPS, 0.0, 0, 0, 0, None, None, None, 5)
    assert rc != 0 and b"null row map" in lib.t4r_last_error()


# ------------------------------------------------------------------------------------------------ model level
def _model(masking):
    import transformers4rec_amd as tr

    V, L, D = 2000, 20, 64
    schema = tr.session_schema(V - 1, L)
    torch.manual_seed(0)
    inputs = tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=L, masking=masking, embedding_dim_default=D)
    cfg = tr.XLNetConfig.build(D, 4, 2, total_seq_length=L, dropout=0.3, initializer_range=0.05)
    return cfg.to_torch_model(inputs, tr.NextItemPredictionTask(weight_tying=True)).to(DEV)


def _step(masking, ids, on):
    from transformers4rec_amd import transformer as tfm

    model = _model(masking)          # same seed: same weights, same Philox keys, same counters
    model.train()
    prev = tfm._LAST_ROWS
    tfm._LAST_ROWS = on
    try:
        out = model({"item_id": ids}, training=True)
        ran = model.transformer_block.transformer.last_out_rows
        out["loss"].backward()
        torch.cuda.synchronize()
    finally:
        tfm._LAST_ROWS = prev
    preds = out["predictions"]
    preds = preds.materialize() if hasattr(preds, "materialize") else preds
    grads = {k: q.grad.detach().clone() for k, q in model.named_parameters() if q.grad is not None}
    return out["loss"].detach().clone(), out["labels"].clone(), preds.detach().clone(), grads, ran, model


def test_model_step_last_rows_on_and_off():
    ids = torch.randint(1, 2000, (64, 20), generator=torch.Generator().manual_seed(3)).to(DEV)
    loss1, lab1, pr1, g1, ran1, model = _step("mlm", ids, True)
    loss0, lab0, pr0, g0, ran0, _ = _step("mlm", ids, False)
    assert ran0 is None and ran1 == model.input_features.masking.n_labels() and 0 < ran1 <= 64 * 20 // 2
    assert torch.equal(loss1, loss0) and torch.equal(lab1, lab0) and torch.equal(pr1, pr0)
    assert set(g1) == set(g0) and len(g1) > 30
    for k in g0:
        close(g1[k].reshape(-1), g0[k].reshape(-1), rtol=2 * GRAD_TOL[0], atol=2 * GRAD_TOL[1], msg=lambda mm, k=k: f"{k}: {mm}")


def test_model_clm_training_takes_the_full_path():
    """labels at nearly every position: the row rule keeps the gate off"""
    ids = torch.randint(1, 2000, (64, 20), generator=torch.Generator().manual_seed(4)).to(DEV)
    loss, _, _, _, ran, model = _step("clm", ids, True)
    assert ran is None and model.input_features.masking.n_labels() > 64 * 20 // 2 and bool(torch.isfinite(loss))
