"""Kernel-level parity: every C-ABI entry point (through transformers4rec_amd.ops, which only
marshals pointers) against the CPU oracle / plain torch fp32 on the same seeded inputs.
Integer outputs bit-exact; fp32 outputs to 1e-5-class tolerances (O(0.1-1) weights)."""
import numpy as np
import pytest
import torch

import golden_utils as gu
import t4r_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from transformers4rec_amd import ops as _ops

    return _ops


def cu(t):
    return t.to(DEV).contiguous()


def close(a, b, rtol=2e-5, atol=2e-5, msg=None):
    torch.testing.assert_close(a.cpu(), b.cpu(), rtol=rtol, atol=atol, msg=msg)


# ------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(128, 128, 128), (77, 130, 33), (300, 64, 512), (33, 1001, 128),
                                   (1, 5, 3), (257, 384, 128)])
def test_gemm_layouts(ops, ta, tb, M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K + ta * 2 + tb)
    A = torch.randn((K, M) if ta else (M, K), generator=g)
    B = torch.randn((N, K) if tb else (K, N), generator=g)
    ref = (A.t() if ta else A).double() @ (B.t() if tb else B).double()
    out = ops.gemm(cu(A), cu(B), bool(ta), bool(tb), alpha=0.5)
    close(out, (0.5 * ref).float(), rtol=1e-5, atol=1e-4)


def test_gemm_asymmetric_identity(ops):
    """A = I with an asymmetric B catches a transposed C write (guide rule 16)."""
    n = 96
    B = torch.arange(n * n, dtype=torch.float32).reshape(n, n) / 100.0
    out = ops.gemm(cu(torch.eye(n)), cu(B))
    assert torch.equal(out.cpu(), B)


def test_gemm_epilogues_splitk_accumulate(ops):
    g = torch.Generator().manual_seed(5)
    M, N, K = 200, 192, 96
    A, W, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    pre = A @ W.t() + bias
    aux = torch.empty((M, N), device=DEV)
    out = ops.gemm(cu(A), cu(W), False, True, bias=cu(bias), epilogue=ops.EPI_BIAS_GELU, aux=aux)
    close(aux, pre, atol=1e-4)
    close(out, torch.nn.functional.gelu(pre), atol=1e-4)
    out = ops.gemm(cu(A), cu(W), False, True, bias=cu(bias), epilogue=ops.EPI_BIAS_RELU)
    close(out, torch.relu(pre), atol=1e-4)
    out = ops.gemm(cu(A), cu(W), False, True, bias=cu(bias), epilogue=ops.EPI_BIAS)
    close(out, pre, atol=1e-4)
    # split-K (atomics): overwrite and accumulate flavours, long K
    K2 = 5000
    A2, B2 = torch.randn(K2, 70, generator=g), torch.randn(K2, 90, generator=g)
    ref = (A2.t().double() @ B2.double()).float()
    out = ops.gemm(cu(A2), cu(B2), True, False, splitk=-1)
    close(out, ref, rtol=1e-4, atol=2e-3)
    acc = cu(torch.ones(70, 90))
    ops.gemm(cu(A2), cu(B2), True, False, splitk=-1, accumulate=True, out=acc)
    close(acc, ref + 1, rtol=1e-4, atol=2e-3)
    acc = cu(torch.ones(70, 90))
    ops.gemm(cu(A2), cu(B2), True, False, splitk=1, accumulate=True, out=acc)
    close(acc, ref + 1, rtol=1e-4, atol=2e-3)
    # padded leading dimension of C and unaligned K (logits-like: N odd)
    X, Wv = torch.randn(37, 64, generator=g), torch.randn(1001, 64, generator=g)
    out = ops.gemm(cu(X), cu(Wv), False, True, alpha=1 / 0.7, ldc=ops.pad_ld(1001))
    assert out.stride(0) == ops.pad_ld(1001) and out.stride(0) % 64 == 0 and out.stride(0) >= 1001
    close(out, (X @ Wv.t()) / 0.7, atol=1e-4)
    # K not a multiple of 4 with a k-contiguous operand and padded lda (head dX shape)
    dl = torch.zeros(37, 1004)
    dl[:, :1001] = torch.randn(37, 1001, generator=g)
    dx = ops.gemm(cu(dl)[:, :1001], cu(Wv), False, False, splitk=-1)
    close(dx, dl[:, :1001] @ Wv, rtol=1e-4, atol=1e-3)


# ------------------------------------------------------------------------------------ LN / act / adam
@pytest.mark.parametrize("rows,D", [(50, 128), (33, 64), (20, 8), (7, 512), (9, 336), (4, 32)])
def test_add_layernorm_fwd_bwd(ops, rows, D):
    g = torch.Generator().manual_seed(rows + D)
    a, b = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g)
    gam, bet = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    dy = torch.randn(rows, D, generator=g)
    a_, b_, g_, be_ = (t.clone().requires_grad_() for t in (a, b, gam, bet))
    ref = O.layer_norm(a_ + b_, g_, be_, 0.03)
    ref.backward(dy)
    y, mean, rstd = ops.add_layernorm_fwd(cu(a), cu(b), cu(gam), cu(bet), 0.03)
    close(y, ref.detach())
    dg, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    dx = ops.add_layernorm_bwd(cu(a), cu(b), cu(gam), mean, rstd, cu(dy), dg, db)
    close(dx, a_.grad, atol=5e-5)
    close(dg, g_.grad, atol=1e-4)
    close(db, be_.grad, atol=1e-4)
    y2, _, _ = ops.add_layernorm_fwd(cu(a), None, cu(gam), cu(bet), 1e-5)
    close(y2, O.layer_norm(a, gam, bet, 1e-5))


def test_act_bwd_bias_and_colsum(ops):
    g = torch.Generator().manual_seed(3)
    pre = torch.randn(100, 96, generator=g).requires_grad_()
    dact = torch.randn(100, 96, generator=g)
    torch.nn.functional.gelu(pre).backward(dact)
    db = torch.zeros(96, device=DEV)
    out = ops.act_bwd_bias(cu(dact), cu(pre.detach()), db, 0, out=torch.empty(100, 96, device=DEV))
    close(out, pre.grad, atol=1e-5)
    close(db, pre.grad.sum(0), atol=1e-4)
    relu_out = torch.relu(pre.detach())
    out = ops.act_bwd_bias(cu(dact), cu(relu_out), None, 1, out=torch.empty(100, 96, device=DEV))
    close(out, dact * (relu_out > 0))
    acc = torch.zeros(96, device=DEV)
    ops.colsum_(cu(dact), acc)
    close(acc, dact.sum(0), atol=1e-4)


def test_adam_matches_torch(ops):
    g = torch.Generator().manual_seed(0)
    n = 4099
    p0, grads = torch.randn(n, generator=g), [torch.randn(n, generator=g) for _ in range(3)]
    p_ref = p0.clone().requires_grad_()
    opt = torch.optim.Adam([p_ref], lr=1e-2, weight_decay=0.01)
    p, m, v = cu(p0.clone()), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for step, gr in enumerate(grads, 1):
        p_ref.grad = gr.clone()
        opt.step()
        gd = cu(2.0 * gr)
        ops.adam_step_(p, gd, m, v, step, lr=1e-2, weight_decay=0.01, grad_scale=0.5)
        assert float(gd.abs().max()) == 0.0  # zero_grad fused
        close(p, p_ref.detach(), rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------ masking (bit exact)
def test_mask_targets_golden_bit_exact(ops):
    d = gu.load("masking_int")
    ids = cu(gu.t(d["in/item_id"]))
    m, lab, cnt = ops.mask_targets(ids, ops.MLM_TRAIN, bern=cu(gu.t(d["draw/bern"])).to(torch.uint8),
                                   j1=cu(gu.t(d["draw/j1"])), j2=cu(gu.t(d["draw/j2"])))
    assert torch.equal(m.cpu(), gu.t(d["out/mask_schema"]))
    assert torch.equal(lab.cpu(), gu.t(d["out/masked_targets"]))
    assert torch.equal(cnt.cpu().long(), (gu.t(d["out/masked_targets"]) != 0).sum(1))
    for mode, tag in ((ops.MLM_EVAL_LAST, "eval_last"), (ops.MLM_EVAL_ALL, "eval_all"), (ops.MLM_INFER, "infer")):
        m, lab, _ = ops.mask_targets(ids, mode)
        assert torch.equal(m.cpu(), gu.t(d[f"out/{tag}_schema"])), tag
        assert torch.equal(lab.cpu(), gu.t(d[f"out/{tag}_targets"])), tag
    ids2 = cu(gu.t(d["in/item_id_clm"]))
    for mode, tag in ((ops.CLM_TRAIN, "clm_train"), (ops.CLM_LAST, "clm_train_last"),
                      (ops.CLM_LAST, "clm_eval_last"), (ops.CLM_TRAIN, "clm_eval_all"),
                      (ops.CLM_INFER, "clm_infer")):
        m, lab, _ = ops.mask_targets(ids2, mode)
        assert torch.equal(m.cpu(), gu.t(d[f"out/{tag}_schema"])), tag
        assert torch.equal(lab.cpu(), gu.t(d[f"out/{tag}_targets"])), tag


@pytest.mark.parametrize("L", [1, 2, 20, 63, 64, 65, 100, 200])
def test_mask_targets_vs_oracle_random(ops, L):
    g = torch.Generator().manual_seed(L)
    B = 70
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0] = L
    ids = torch.randint(1, 999, (B, L), generator=g) * (torch.arange(L)[None] < lens[:, None])
    bern = torch.rand(B, L, generator=g) < 0.5
    j1 = (torch.rand(B, generator=g) * lens).long()
    m0 = bern & (ids != 0)
    j2 = torch.zeros(B, dtype=torch.int64)
    ref_m, ref_l = O.mlm_targets_train(ids, bern, j1, lambda mm: mm.float().argmax(1))
    # feed the same j2 the lambda produced
    tmp = torch.where(m0, ids, torch.zeros_like(ids)); tmp[torch.arange(B), j1] = ids[torch.arange(B), j1]
    j2 = (tmp != 0).float().argmax(1)
    m, lab, _ = ops.mask_targets(cu(ids), ops.MLM_TRAIN, bern=cu(bern).to(torch.uint8), j1=cu(j1), j2=cu(j2))
    assert torch.equal(m.cpu(), ref_m) and torch.equal(lab.cpu(), ref_l)
    for mode, fn in ((ops.MLM_EVAL_LAST, lambda: O.mlm_targets_eval(ids, True)),
                     (ops.MLM_EVAL_ALL, lambda: O.mlm_targets_eval(ids, False)),
                     (ops.MLM_INFER, lambda: O.mlm_targets_inference(ids)),
                     (ops.CLM_TRAIN, lambda: O.clm_targets(ids, True, False)),
                     (ops.CLM_LAST, lambda: O.clm_targets(ids, False, True)),
                     (ops.CLM_INFER, lambda: O.clm_targets(ids, False, False))):
        if L == 1 and mode == ops.CLM_LAST:
            continue  # reference indexes labels[-1] on an all-pad label row; same wrap, covered at L>=2
        rm, rl = fn()
        m, lab, _ = ops.mask_targets(cu(ids), mode)
        assert torch.equal(m.cpu(), rm), mode
        assert torch.equal(lab.cpu(), rl), mode


def test_mask_targets_device_rng_invariants(ops):
    """Reference invariants (tests/unit/torch/test_masking.py:117-150) on the Philox path."""
    g = torch.Generator().manual_seed(1)
    B, L = 4096, 20
    lens = torch.randint(1, L + 1, (B,), generator=g)
    ids = cu(torch.randint(1, 999, (B, L), generator=g) * (torch.arange(L)[None] < lens[:, None]))
    m, lab, cnt = ops.mask_targets(ids, ops.MLM_TRAIN, p=0.15, seed=123, offset=0)
    m2, lab2, _ = ops.mask_targets(ids, ops.MLM_TRAIN, p=0.15, seed=123, offset=0)
    assert torch.equal(m, m2) and torch.equal(lab, lab2)  # deterministic in (seed, offset)
    m3, _, _ = ops.mask_targets(ids, ops.MLM_TRAIN, p=0.15, seed=124, offset=0)
    assert not torch.equal(m, m3)
    nonpad = ids != 0
    n_lab, n_np = m.sum(1), nonpad.sum(1)
    assert bool((m & ~nonpad).sum() == 0)
    assert bool(torch.equal(lab, torch.where(m, ids, torch.zeros_like(ids))))
    assert bool(((n_lab >= 1) | (n_np == 1)).all())          # >= 1 label unless a 1-item session
    assert bool(((n_lab < n_np) | (n_np == 0)).all())         # never all items masked
    assert torch.equal(cnt.long(), n_lab)
    frac = float(m.sum()) / float(nonpad.sum())
    assert 0.15 < frac < 0.30                                 # p=0.15 plus the forced label


def test_compact_gather_scatter(ops):
    g = torch.Generator().manual_seed(2)
    B, L, D = 1500, 20, 64
    labels = torch.randint(0, 50, (B, L), generator=g) * (torch.rand(B, L, generator=g) < 0.2)
    x = torch.randn(B, L, D, generator=g)
    ref_x, ref_y = O.remove_pad_rows(x, labels)
    lab_d = cu(labels)
    cnt = (lab_d != 0).sum(1).to(torch.int32)
    n, pos, lab = ops.compact_labels(lab_d, cnt)
    N = int(n.item())
    assert N == ref_y.numel()
    assert torch.equal(lab[:N].cpu(), ref_y)
    out = ops.gather_rows(cu(x).view(B * L, D), pos, N)
    assert torch.equal(out.cpu(), ref_x)
    dx = torch.zeros(B * L, D, device=DEV)
    ops.scatter_rows_add_(out, pos, dx)
    ref_dx = torch.zeros(B * L, D)
    ref_dx[(labels.flatten() != 0)] = ref_x
    assert torch.equal(dx.cpu(), ref_dx)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    ids = torch.where(torch.arange(L)[None] < lens[:, None], 5, 0)
    pos_mlm = ops.last_positions(cu(ids), L + 1, True)
    assert torch.equal(pos_mlm.cpu().long(), torch.arange(B) * (L + 1) + lens)
    pos_clm = ops.last_positions(cu(ids), L, False)
    assert torch.equal(pos_clm.cpu().long(), torch.arange(B) * L + lens - 1)


def test_ragged_to_padded_golden(ops):
    d = gu.load("padding")
    vals, fvals, offs = cu(gu.t(d["in/values"])), cu(gu.t(d["in/fvalues"])), cu(gu.t(d["in/offsets"]))
    mx = int(ops.ragged_max_len(offs).item())
    assert mx == int((gu.t(d["in/offsets"])[1:] - gu.t(d["in/offsets"])[:-1]).max())
    for msl in (None, 20, 64):
        L = mx if msl is None else min(msl, mx)
        assert torch.equal(ops.ragged_to_padded(vals, offs, L).cpu(), gu.t(d[f"out/pad_inputs_{msl}_a"]))
        assert torch.equal(ops.ragged_to_padded(fvals, offs, L).cpu(), gu.t(d[f"out/pad_inputs_{msl}_f"]))
    assert torch.equal(ops.ragged_to_padded(vals, offs, 7).cpu(), gu.t(d["out/pad_batch_7"]))
    assert torch.equal(ops.ragged_to_padded(vals, offs, 45).cpu(), gu.t(d["out/pad_batch_45"]))
    # reference known answers (tests/unit/utils/test_padding.py:33-80): empty row + truncation
    v = cu(torch.tensor([1, 2, 3, 4, 5, 4, 7]))
    o = cu(torch.tensor([0, 2, 2, 7]))
    assert ops.ragged_to_padded(v, o, 3).cpu().tolist() == [[1, 2, 0], [0, 0, 0], [3, 4, 5]]


# ------------------------------------------------------------------------------------ input block
def _feat_setup(g, B, L, dims, cards):
    lens = torch.randint(1, L + 1, (B,), generator=g)
    m = torch.arange(L)[None] < lens[:, None]
    ids = [torch.randint(1, c, (B, L), generator=g) * m for c in cards]
    tabs = [torch.randn(c, d, generator=g) for c, d in zip(cards, dims)]
    return ids, tabs


@pytest.mark.parametrize("dims", [(128,), (64, 24, 8), (16, 12, 6), (32, 32, 32),
                                  (128, 64, 64, 64, 8, 8),        # C3's 336-wide row: fast path, 2 chunks per lane
                                  (256, 200, 128, 64), (512, 512)])  # 648- and 1024-wide rows: 3-4 chunks per lane
def test_seq_features_concat_and_mask_modes(ops, dims):
    g = torch.Generator().manual_seed(sum(dims))
    B, L = 37, 20
    cards = [500, 40, 9, 77, 13, 300][: len(dims)]
    ids, tabs = _feat_setup(g, B, L, dims, cards)
    cols = np.cumsum([0] + list(dims))
    W = int(cols[-1])
    feats = [dict(kind=0, input=cu(i), table=cu(t), dim=d, col=int(c), rows=t.shape[0])
             for i, t, d, c in zip(ids, tabs, dims, cols)]
    ref = torch.cat([O.embedding_lookup(i, t) for i, t in zip(ids, tabs)], -1)
    out = ops.seq_features_fwd(feats, "concat", B, L, L, W)
    assert torch.equal(out.cpu(), ref)
    memb = torch.randn(W, generator=g)
    mask = torch.rand(B, L, generator=g) < 0.3
    out = ops.seq_features_fwd(feats, "concat", B, L, L, W, mask_mode=ops.MASK_MLM, mask=cu(mask), masked_emb=cu(memb))
    assert torch.equal(out.cpu(), O.apply_mask_mlm(ref, mask, memb, True, False))
    out = ops.seq_features_fwd(feats, "concat", B, L, L, W, mask_mode=ops.MASK_CLM, mask=cu(mask), masked_emb=cu(memb))
    assert torch.equal(out.cpu(), O.apply_mask_clm(ref, mask, memb, True, False))
    out = ops.seq_features_fwd(feats, "concat", B, L, L, W, mask_mode=ops.MASK_CLM_INFER, mask=cu(mask), masked_emb=cu(memb))
    assert torch.equal(out.cpu(), O.apply_mask_clm(ref, mask, memb, False, False))
    mask1 = torch.rand(B, L + 1, generator=g) < 0.3
    out = ops.seq_features_fwd(feats, "concat", B, L, L + 1, W, mask_mode=ops.MASK_MLM, mask=cu(mask1), masked_emb=cu(memb))
    assert torch.equal(out.cpu(), O.apply_mask_mlm(ref, mask1, memb, False, False))
    # separate-pass masking
    x = cu(ref.clone())
    ops.apply_mask_fwd_(x, cu(mask), cu(memb), ops.MASK_MLM)
    assert torch.equal(x.cpu(), O.apply_mask_mlm(ref, mask, memb, True, False))
    x = cu(ref.clone())
    ops.apply_mask_fwd_(x, cu(mask), cu(memb), ops.MASK_CLM)
    assert torch.equal(x.cpu(), O.apply_mask_clm(ref, mask, memb, True, False))
    # backward of masking + gather against autograd
    for mode, fn in ((ops.MASK_MLM, O.apply_mask_mlm), (ops.MASK_CLM, O.apply_mask_clm)):
        tabs_r = [t.clone().requires_grad_() for t in tabs]
        memb_r = memb.clone().requires_grad_()
        y = fn(torch.cat([O.embedding_lookup(i, t) for i, t in zip(ids, tabs_r)], -1), mask, memb_r, True, False)
        dy = torch.randn(y.shape, generator=g)
        y.backward(dy)
        dyd = cu(dy.clone())
        dm = torch.zeros(W, device=DEV)
        ops.apply_mask_bwd_(dyd, cu(mask), dm, mode)
        close(dm, memb_r.grad, atol=1e-4)
        for i, t, tr, d, c in zip(ids, tabs, tabs_r, dims, cols):
            dt = torch.zeros(t.shape, device=DEV)
            ops.embedding_bwd(dyd, cu(i), dt, int(c), d)
            close(dt, tr.grad, atol=1e-4)


def test_seq_features_sum_and_item_multi(ops):
    g = torch.Generator().manual_seed(9)
    B, L, D = 21, 20, 32
    ids, tabs = _feat_setup(g, B, L, (D, D, D), (300, 40, 7))
    feats = [dict(kind=0, input=cu(i), table=cu(t), dim=D, col=0, rows=t.shape[0]) for i, t in zip(ids, tabs)]
    embs = {f"f{k}": O.embedding_lookup(i, t) for k, (i, t) in enumerate(zip(ids, tabs))}
    out = ops.seq_features_fwd(feats, "element-wise-sum", B, L, L, D)
    close(out, O.elementwise_sum(embs), atol=1e-6)
    out = ops.seq_features_fwd(feats, "element-wise-sum-item-multi", B, L, L, D, item_feat=0)
    close(out, O.elementwise_sum_item_multi(embs, "f0"), atol=1e-6)
    # dense (kind 1) feature rows mixed in a concat
    dense = torch.randn(B, L, 8, generator=g)
    feats2 = [dict(kind=0, input=cu(ids[0]), table=cu(tabs[0]), dim=D, col=8, rows=300),
              dict(kind=1, input=cu(dense), table=None, dim=8, col=0)]
    out = ops.seq_features_fwd(feats2, "concat", B, L, L, D + 8)
    assert torch.equal(out.cpu(), torch.cat([dense, embs["f0"]], -1))
    err = torch.zeros(1, device=DEV, dtype=torch.int32)
    bad = cu(ids[0].clone()); bad[0, 0] = 10 ** 6
    ops.seq_features_fwd([dict(kind=0, input=bad, table=cu(tabs[0]), dim=D, col=0, rows=300)], "concat",
                         B, L, L, D, err_flag=err)
    assert int(err.item()) == 1


@pytest.mark.parametrize("K,D,ln", [(10, 8, True), (10, 8, False), (20, 16, True)])
def test_soft_embedding_fwd_bwd(ops, K, D, ln):
    g = torch.Generator().manual_seed(K + D)
    B, L = 33, 20
    x = torch.rand(B, L, generator=g)
    pw, pb, tab = (torch.randn(K, 1, generator=g), torch.randn(K, generator=g), torch.randn(K, D, generator=g))
    lw, lb = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    ps = [t.clone().requires_grad_() for t in (pw, pb, tab, lw, lb)]
    ref = O.soft_embedding(x, ps[0], ps[1], ps[2])
    if ln:
        ref = O.layer_norm(ref, ps[3], ps[4], 1e-5)
    dy = torch.randn(B, L, D + 4, generator=g)
    ref.backward(dy[..., 4:])
    out = ops.soft_embedding_fwd(cu(x), cu(pw), cu(pb), cu(tab), cu(lw) if ln else None, cu(lb) if ln else None)
    close(out, ref.detach(), atol=1e-5)
    gr = [torch.zeros(t.shape, device=DEV) for t in (pw, pb, tab, lw, lb)]
    ops.soft_embedding_bwd(cu(dy), cu(x), cu(pw), cu(pb), cu(tab), cu(lw) if ln else None, gr[0], gr[1], gr[2],
                           gr[3] if ln else None, gr[4] if ln else None, col=4)
    for got, p in zip(gr[: (5 if ln else 3)], ps):
        close(got, p.grad, rtol=1e-4, atol=2e-4)


# ------------------------------------------------------------------------------------ attention / layer
def _layer_params(g, D, n, scale=0.1):
    dh = D // n
    r = lambda *s: scale * torch.randn(*s, generator=g)
    return dict(q=r(D, n, dh), k=r(D, n, dh), v=r(D, n, dh), o=r(D, n, dh), r=r(D, n, dh),
                r_w_bias=r(n, dh), r_r_bias=r(n, dh), ln_w=1 + r(D), ln_b=r(D),
                w1=r(4 * D, D), b1=r(4 * D), w2=r(D, 4 * D), b2=r(D), ff_ln_w=1 + r(D), ff_ln_b=r(D))


ORDER = ("q", "k", "v", "o", "r", "r_w_bias", "r_r_bias", "ln_w", "ln_b", "w1", "b1", "w2", "b2",
         "ff_ln_w", "ff_ln_b")


@pytest.mark.parametrize("B,L,D,n", [(5, 20, 64, 4), (3, 21, 32, 2), (2, 7, 128, 4), (4, 33, 64, 8), (2, 64, 32, 2),
                                     (3, 32, 128, 4), (2, 1, 64, 2), (1100, 5, 32, 1), (4, 17, 16, 1), (2, 32, 32, 2),
                                     # beyond one wave (csrc/xlnet_attn_long.hip): d_head 16, 16, 64, 8, 32; row blocks 2 .. 4
                                     (2, 65, 32, 2), (3, 100, 64, 4), (2, 130, 128, 2), (1, 200, 16, 2), (1030, 70, 32, 1),
                                     # head widths without a one-wave instance: 48, 64, 128, 24, 12, 40
                                     (3, 20, 96, 2), (2, 33, 256, 4), (2, 20, 256, 2), (2, 100, 48, 2), (2, 20, 24, 2), (5, 9, 40, 1),
                                     # one-wave shapes whose K / V / k_r rows do not fit the LDS of the VALU kernels
                                     (2, 50, 256, 8), (2, 64, 512, 16), (3, 40, 512, 32),
                                     # d_head 160, 256 (per-thread vectors in scratch)
                                     (2, 20, 320, 2), (2, 70, 256, 1),
                                     # head widths that are not a multiple of 4: 25, 25, 10
                                     (3, 20, 100, 4), (2, 70, 50, 2), (2, 9, 20, 2)])
def test_xlnet_attention_core(ops, B, L, D, n):
    g = torch.Generator().manual_seed(B * L + D)
    dh = D // n
    q, k, v = (torch.randn(B, L, n, dh, generator=g).requires_grad_() for _ in range(3))
    kr = torch.randn(2 * L, n, dh, generator=g).requires_grad_()
    rw, rr = (0.5 * torch.randn(n, dh, generator=g)).requires_grad_(), (0.5 * torch.randn(n, dh, generator=g)).requires_grad_()
    ac = torch.einsum("bind,bjnd->bnij", q + rw, k)
    bd_full = torch.einsum("bind,pnd->bnip", q + rr, kr)
    idx = torch.arange(L)[None, :] + L - torch.arange(L)[:, None]
    bd = torch.gather(bd_full, 3, idx[None, None].expand(B, n, L, L))
    prob = torch.softmax((ac + bd) / dh ** 0.5, 3)
    ref = torch.einsum("bnij,bjnd->bind", prob, v)
    dout = torch.randn(B, L, n, dh, generator=g)
    ref.backward(dout)
    f2 = lambda t: cu(t.detach().reshape(-1, D))
    out, lse = ops.xlnet_attn_fwd(f2(q), f2(k), f2(v), f2(kr), cu(rw.detach().reshape(-1)), cu(rr.detach().reshape(-1)), B, L, n)
    close(out, ref.detach().reshape(-1, D), atol=2e-5)
    drw, drr = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    dq, dk, dv, dkr = ops.xlnet_attn_bwd(f2(q), f2(k), f2(v), f2(kr), cu(rw.detach().reshape(-1)),
                                         cu(rr.detach().reshape(-1)), out, lse, f2(dout), drw, drr, B, L, n)
    close(dq, q.grad.reshape(-1, D), atol=1e-4)
    close(dk, k.grad.reshape(-1, D), atol=1e-4)
    close(dv, v.grad.reshape(-1, D), atol=1e-4)
    close(dkr, kr.grad.reshape(-1, D), atol=2e-4)
    close(drw, rw.grad.reshape(-1), atol=3e-4)
    close(drr, rr.grad.reshape(-1), atol=3e-4)


@pytest.mark.parametrize("B,L,D,n", [(6, 20, 64, 4), (3, 21, 32, 2), (9, 20, 128, 4)])
def test_xlnet_layer_fwd_bwd(ops, B, L, D, n):
    g = torch.Generator().manual_seed(B + L + D)
    p = _layer_params(g, D, n)
    pr = {k: v.clone().requires_grad_() for k, v in p.items()}
    h = torch.randn(B, L, D, generator=g)
    hr = h.clone().requires_grad_()
    ref = O.xlnet_layer(hr, pr, n, 0.03)
    dout = torch.randn(B, L, D, generator=g)
    ref.backward(dout)
    pos = cu(O.xlnet_pos_emb(L, D))
    params = [cu(p[k]) for k in ORDER]
    out, ws = ops.xlnet_layer_fwd(cu(h).view(B * L, D), pos, params, B, L, n, 0.03)
    close(out, ref.detach().reshape(B * L, D), atol=3e-5)
    grads = [torch.zeros_like(t) for t in params]
    dh = ops.xlnet_layer_bwd(cu(h).view(B * L, D), pos, params, grads, ws, cu(dout).view(B * L, D), B, L, n, 0.03)
    close(dh, hr.grad.reshape(B * L, D), rtol=1e-4, atol=2e-4)
    for k, gt in zip(ORDER, grads):
        close(gt.reshape(-1), pr[k].grad.reshape(-1), rtol=1e-4, atol=5e-4, msg=lambda m, k=k: f"{k}: {m}")


def test_xlnet_layer_golden_hidden(ops):
    """reference fixture: inputs_embeds -> hidden through both layers."""
    d = gu.load("xlnet_mlm_item_train")
    p = gu.oracle_params(d)
    x = gu.t(d["out/inputs_embeds"])
    B, L, D = x.shape
    n = int(d["meta/n_head"])
    pos = cu(O.xlnet_pos_emb(L, D))
    h = cu(x).view(B * L, D)
    for lp in p["layers"]:
        params = [cu(lp[k]) for k in ORDER]
        h, _ = ops.xlnet_layer_fwd(h, pos, params, B, L, n, float(d["meta/eps"]))
    close(h.view(B, L, D), gu.t(d["out/hidden"]), atol=3e-5)


# ------------------------------------------------------------------------------------ head
@pytest.mark.parametrize("N,V,eps", [(37, 1001, 0.0), (5, 100001, 0.0), (16, 517, 0.1), (1, 33, 0.0)])
def test_softmax_ce_fwd_bwd(ops, N, V, eps):
    g = torch.Generator().manual_seed(N + V)
    ld = ops.pad_ld(V)
    logits = 3 * torch.randn(N, V, generator=g)
    y = torch.randint(0, V, (N,), generator=g)
    lr = logits.clone().requires_grad_()
    ref = torch.nn.functional.cross_entropy(lr, y, label_smoothing=eps)
    (ref * 1.7).backward()
    buf = torch.zeros(N, ld, device=DEV)
    buf[:, :V] = cu(logits)
    loss, rows, lse = ops.softmax_ce_fwd(buf[:, :V], cu(y), V, eps)
    close(loss, ref.detach(), atol=1e-5)
    dl = ops.softmax_ce_bwd(buf[:, :V], cu(y), lse, torch.tensor(1.7, device=DEV), V, eps)
    close(dl[:, :V], lr.grad, rtol=1e-4, atol=1e-7)
    assert float(dl[:, V:].abs().sum()) == 0.0


def test_sampled_logits_golden(ops):
    d = gu.load("xlnet_mlm_sum_sampled_train")
    p = gu.oracle_params(d, requires_grad=True)
    n = int(d["meta/max_n_samples"])
    neg = gu.t(d["draw/neg_tries"]).unique()[:n]
    dist = gu.section(d, "p/")[gu.TASK + "pre.module.sampler.unique_sampling_dist"]
    j2 = gu.t(d["draw/j2"])
    _, lab = O.mlm_targets_train(gu.t(d["in/item_id"]), gu.t(d["draw/bern"]), gu.t(d["draw/j1"]), lambda m: j2)
    xr, y = O.remove_pad_rows(gu.t(d["out/hidden"]), lab)
    W = p["tables"]["item_id"]
    xr_ = xr.clone().requires_grad_()
    ref = O.sampled_logits(xr_, y, W, neg, dist)
    close(ref.detach(), gu.t(d["out/predictions"]), atol=1e-4)
    out = ops.sampled_logits_fwd(cu(xr), cu(y), cu(W.detach()), cu(neg), cu(dist))
    close(out, ref.detach(), atol=1e-4)
    dl = torch.randn(ref.shape, generator=torch.Generator().manual_seed(0))
    ref.backward(dl)
    dW = torch.zeros(W.shape, device=DEV)
    dx = ops.sampled_logits_bwd(cu(dl), cu(xr), cu(y), cu(W.detach()), cu(neg), dW)
    close(dx, xr_.grad, atol=1e-4)
    close(dW, W.grad, atol=1e-4)


@pytest.mark.parametrize("N,V,k", [(9, 1000, 20), (3, 100001, 20), (4, 50, 10), (2, 64, 64), (3, 100001, 100), (2, 5000, 256),
                                   (2, 300, 200)])
def test_topk(ops, N, V, k):
    g = torch.Generator().manual_seed(V)
    s = torch.randn(N, V, generator=g)
    ref_v, ref_i = torch.topk(s, k, dim=-1)
    v, i = ops.topk(cu(s), k)
    assert torch.equal(v.cpu(), ref_v)
    assert torch.equal(i.cpu(), ref_i)


# ------------------------------------------------------------------------------------ dropout
def _mask(ops, shape, p, seed, ctr):
    n = int(np.prod(shape))
    _, m = ops.dropout(torch.ones(1, device=DEV), p, seed, ctr, n_total=n, want_mask=True)
    return m.view(shape).float().cpu()


def test_dropout_mask_properties(ops):
    n, p = 1 << 20, 0.3
    x = torch.randn(n, device=DEV)
    out, m = ops.dropout(x, p, 7, ops.dropout_ctr_hi(1, 0, 3), want_mask=True)
    keep = m.float().mean().item()
    assert abs(keep - 0.7) < 3e-3
    close(out, x * m / 0.7, atol=1e-6)
    out2 = ops.dropout(x, p, 7, ops.dropout_ctr_hi(1, 0, 3))
    assert torch.equal(out, out2)                                   # pure function of (seed, ctr, idx)
    for other in ((8, ops.dropout_ctr_hi(1, 0, 3)), (7, ops.dropout_ctr_hi(2, 0, 3)),
                  (7, ops.dropout_ctr_hi(1, 1, 3)), (7, ops.dropout_ctr_hi(1, 0, 4))):
        _, m2 = ops.dropout(x, p, other[0], other[1], want_mask=True)
        agree = (m2 == m).float().mean().item()
        assert 0.55 < agree < 0.61                                  # independent masks: 0.7^2 + 0.3^2 = 0.58
    # broadcast source (pos_emb over the batch): every replica gets its own mask
    src = torch.randn(640, device=DEV)
    out, m = ops.dropout(src, p, 1, 5, n_total=640 * 50, want_mask=True)
    close(out.view(50, 640), src[None] * m.view(50, 640) / 0.7, atol=1e-6)
    assert not torch.equal(m.view(50, 640)[0], m.view(50, 640)[1])
    assert torch.equal(ops.dropout(x, 0.0, 1, 1), x)


@pytest.mark.parametrize("rows,D", [(50, 128), (33, 64), (7, 512)])
def test_add_layernorm_dropout_fwd_bwd(ops, rows, D):
    g = torch.Generator().manual_seed(rows * D)
    p, seed, ctr = 0.3, 11, ops.dropout_ctr_hi(5, 2, ops.SITE_ATTN_OUT)
    a, b = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g)
    gam, bet = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    dy = torch.randn(rows, D, generator=g)
    m = _mask(ops, (rows, D), p, seed, ctr)
    a_, b_, g_, be_ = (t.clone().requires_grad_() for t in (a, b, gam, bet))
    ref = O.layer_norm(a_ * m / (1 - p) + b_, g_, be_, 0.03)
    ref.backward(dy)
    y, mean, rstd = ops.add_layernorm_fwd(cu(a), cu(b), cu(gam), cu(bet), 0.03, drop=(p, seed, ctr))
    close(y, ref.detach())
    dg, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    dx, dxa = ops.add_layernorm_bwd(cu(a), cu(b), cu(gam), mean, rstd, cu(dy), dg, db, drop=(p, seed, ctr))
    close(dx, b_.grad, atol=5e-5)
    close(dxa, a_.grad, atol=5e-5)
    close(dg, g_.grad, atol=1e-4)


def test_act_bwd_dropout(ops):
    g = torch.Generator().manual_seed(4)
    rows, N, p, seed, ctr = 70, 256, 0.3, 3, ops.dropout_ctr_hi(9, 1, ops.SITE_FF_ACT)
    pre = torch.randn(rows, N, generator=g).requires_grad_()
    dact = torch.randn(rows, N, generator=g)
    m = _mask(ops, (rows, N), p, seed, ctr)
    (torch.nn.functional.gelu(pre) * m / (1 - p)).backward(dact)
    db = torch.zeros(N, device=DEV)
    out = ops.act_bwd_bias(cu(dact), cu(pre.detach()), db, 0, out=torch.empty(rows, N, device=DEV), drop=(p, seed, ctr))
    close(out, pre.grad, atol=1e-5)
    close(db, pre.grad.sum(0), atol=1e-4)


@pytest.mark.parametrize("B,L,D,n", [(5, 20, 64, 4), (3, 21, 128, 4), (4, 9, 32, 2), (2, 32, 64, 2), (1030, 3, 32, 1),
                                     (3, 100, 64, 4), (2, 70, 128, 2), (1030, 66, 16, 1), (3, 20, 192, 4), (2, 40, 256, 2),
                                     (2, 50, 256, 8), (2, 48, 512, 16), (3, 20, 100, 4)])
def test_xlnet_attention_dropout_per_session_kr(ops, B, L, D, n):
    g = torch.Generator().manual_seed(B + L + D)
    dh = D // n
    p, seed, ctr = 0.3, 21, ops.dropout_ctr_hi(2, 1, ops.SITE_PROB)
    q, k, v = (torch.randn(B, L, n, dh, generator=g).requires_grad_() for _ in range(3))
    kr = torch.randn(B, 2 * L, n, dh, generator=g).requires_grad_()
    rw, rr = (0.5 * torch.randn(n, dh, generator=g)).requires_grad_(), (0.5 * torch.randn(n, dh, generator=g)).requires_grad_()
    m = _mask(ops, (B, n, L, L), p, seed, ctr)
    ac = torch.einsum("bind,bjnd->bnij", q + rw, k)
    bd_full = torch.einsum("bind,bpnd->bnip", q + rr, kr)
    idx = torch.arange(L)[None, :] + L - torch.arange(L)[:, None]
    bd = torch.gather(bd_full, 3, idx[None, None].expand(B, n, L, L))
    prob = torch.softmax((ac + bd) / dh ** 0.5, 3) * m / (1 - p)
    ref = torch.einsum("bnij,bjnd->bind", prob, v)
    dout = torch.randn(B, L, n, dh, generator=g)
    ref.backward(dout)
    f2 = lambda t: cu(t.detach().reshape(-1, D))
    rwd, rrd = cu(rw.detach().reshape(-1)), cu(rr.detach().reshape(-1))
    out, lse = ops.xlnet_attn_fwd(f2(q), f2(k), f2(v), f2(kr), rwd, rrd, B, L, n, drop=(p, seed, ctr))
    close(out, ref.detach().reshape(-1, D), atol=3e-5)
    drw, drr = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    dq, dk, dv, dkr = ops.xlnet_attn_bwd(f2(q), f2(k), f2(v), f2(kr), rwd, rrd, out, lse, f2(dout), drw, drr,
                                         B, L, n, drop=(p, seed, ctr))
    close(dq, q.grad.reshape(-1, D), atol=2e-4)
    close(dk, k.grad.reshape(-1, D), atol=2e-4)
    close(dv, v.grad.reshape(-1, D), atol=2e-4)
    close(dkr, kr.grad.reshape(-1, D), atol=2e-4)
    close(drw, rw.grad.reshape(-1), atol=5e-4)
    close(drr, rr.grad.reshape(-1), atol=5e-4)


@pytest.mark.parametrize("B,L,D,n", [(6, 20, 64, 4), (9, 20, 128, 4)])
def test_xlnet_layer_dropout_fwd_bwd(ops, B, L, D, n):
    """whole layer in training mode vs the oracle fed with the SAME masks (extracted per site)."""
    g = torch.Generator().manual_seed(B * 3 + D)
    p_drop, seed, offset, layer = 0.3, 99, 7, 2
    prm = _layer_params(g, D, n)
    pr = {k: v.clone().requires_grad_() for k, v in prm.items()}
    h = torch.randn(B, L, D, generator=g)
    hr = h.clone().requires_grad_()
    C = lambda site: ops.dropout_ctr_hi(offset, layer, site)
    # the pos_emb mask is drawn once per forward and shared by every layer (HF modeling_xlnet.py:1143):
    # its counter carries layer 255, not the layer index
    masks = dict(pos=_mask(ops, (B, 2 * L, D), p_drop, seed, ops.dropout_ctr_hi(offset, 255, ops.SITE_POS)),
                 prob=_mask(ops, (B, n, L, L), p_drop, seed, C(ops.SITE_PROB)),
                 attn_out=_mask(ops, (B, L, D), p_drop, seed, C(ops.SITE_ATTN_OUT)),
                 ff_act=_mask(ops, (B, L, 4 * D), p_drop, seed, C(ops.SITE_FF_ACT)),
                 ff_out=_mask(ops, (B, L, D), p_drop, seed, C(ops.SITE_FF_OUT)))
    ref = O.xlnet_layer_dropout(hr, pr, n, 0.03, masks, p_drop)
    dout = torch.randn(B, L, D, generator=g)
    ref.backward(dout)
    pos = cu(O.xlnet_pos_emb(L, D))
    params = [cu(prm[k]) for k in ORDER]
    kw = dict(drop_p=p_drop, seed=seed, offset=offset, layer_idx=layer)
    out, ws = ops.xlnet_layer_fwd(cu(h).view(B * L, D), pos, params, B, L, n, 0.03, **kw)
    close(out, ref.detach().reshape(B * L, D), atol=5e-5)
    grads = [torch.zeros_like(t) for t in params]
    dh = ops.xlnet_layer_bwd(cu(h).view(B * L, D), pos, params, grads, ws, cu(dout).view(B * L, D), B, L, n, 0.03, **kw)
    close(dh, hr.grad.reshape(B * L, D), rtol=1e-4, atol=3e-4)
    for k, gt in zip(ORDER, grads):
        close(gt.reshape(-1), pr[k].grad.reshape(-1), rtol=1e-4, atol=8e-4, msg=lambda mm, k=k: f"{k}: {mm}")
    # the dropped positional encoding handed in by the caller (drawn once per forward, shared by the layers):
    # bit-identical to the layer drawing its own copy
    pe_b = ops.xlnet_pos_emb_dropout(pos, B, p_drop, seed, offset)
    out2, ws2 = ops.xlnet_layer_fwd(cu(h).view(B * L, D), pos, params, B, L, n, 0.03, pos_emb_b=pe_b, **kw)
    assert torch.equal(out2, out)
    grads2 = [torch.zeros_like(t) for t in params]
    dh2 = ops.xlnet_layer_bwd(cu(h).view(B * L, D), pos, params, grads2, ws2, cu(dout).view(B * L, D), B, L, n, 0.03,
                              pos_emb_b=pe_b, **kw)
    close(dh2, dh, rtol=0, atol=1e-6)
    close(grads2[ORDER.index("r")], grads[ORDER.index("r")], rtol=1e-5, atol=1e-6)


def test_xlnet_layer_backward_is_bit_reproducible(ops):
    """ADVICE / VERDICT r2 #12: the split-K weight gradients no longer use fp32 atomics inside the layer backward (partial
    tiles + one fixed-order reduction, csrc/gemm_f32.hip: t4r_splitk_sink_*): at a size where every weight gradient IS
    split (T = 10 240 tokens), repeated calls give the same bits for every parameter gradient and for d h."""
    B, L, D, n = 512, 20, 128, 4
    g = torch.Generator().manual_seed(5)
    prm = _layer_params(g, D, n)
    h = cu(torch.randn(B * L, D, generator=g))
    dout = cu(torch.randn(B * L, D, generator=g))
    pos = cu(O.xlnet_pos_emb(L, D))
    params = [cu(prm[k]) for k in ORDER]
    kw = dict(drop_p=0.3, seed=11, offset=3, layer_idx=1)
    runs = []
    for _ in range(3):
        out, ws = ops.xlnet_layer_fwd(h, pos, params, B, L, n, 0.03, **kw)
        grads = [torch.zeros_like(t) for t in params]
        dh = ops.xlnet_layer_bwd(h, pos, params, grads, ws, dout, B, L, n, 0.03, **kw)
        torch.cuda.synchronize()
        runs.append([dh.clone()] + [gt.clone() for gt in grads])
    for other in runs[1:]:
        for name, a, b in zip(("dh",) + ORDER, runs[0], other):
            assert torch.equal(a, b), f"{name}: gradients differ between identical calls (max |d| {float((a - b).abs().max()):.3e})"
    assert all(float(t.abs().max()) > 0 for t in runs[0])


@pytest.mark.parametrize("p_drop", [0.0, 0.3])
def test_xlnet_layer_unfused_backward_is_bit_reproducible_and_right(ops, p_drop):
    """The same for the UNFUSED chain (d_model 48 has no token-tile kernels; d_head 16: the one-wave attention kernels): T = 800
    tokens, so every weight gradient is split at least in two and goes through the layer's split-K sink, and the second stages of
    the LayerNorm / bias / attention-bias sums go through the same sink or the side stream.  Three calls give the same bits, and
    one of them is right against the fp64 oracle at the tolerances of test_xlnet_layer_fwd_bwd (p = 0) and
    test_xlnet_layer_dropout_fwd_bwd (p = 0.3)."""
    B, L, D, n = 40, 20, 48, 3
    g = torch.Generator().manual_seed(B + L + D)
    prm = _layer_params(g, D, n)
    h, dout = torch.randn(B, L, D, generator=g), torch.randn(B, L, D, generator=g)
    seed, offset, layer = 99, 7, 2
    kw = dict(drop_p=p_drop, seed=seed, offset=offset, layer_idx=layer) if p_drop else {}
    pos = cu(O.xlnet_pos_emb(L, D))
    params = [cu(prm[k]) for k in ORDER]
    hd, dd = cu(h).view(B * L, D), cu(dout).view(B * L, D)
    runs = []
    for _ in range(3):
        out, ws = ops.xlnet_layer_fwd(hd, pos, params, B, L, n, 0.03, **kw)
        grads = [torch.zeros_like(t) for t in params]
        dh = ops.xlnet_layer_bwd(hd, pos, params, grads, ws, dd, B, L, n, 0.03, **kw)
        torch.cuda.synchronize()
        runs.append([dh.clone()] + [gt.clone() for gt in grads])
    for other in runs[1:]:
        for name, a, b in zip(("dh",) + ORDER, runs[0], other):
            assert torch.equal(a, b), f"{name}: gradients differ between identical calls (max |d| {float((a - b).abs().max()):.3e})"
    pr = {k: v.double().requires_grad_() for k, v in prm.items()}
    hr = h.double().requires_grad_()
    if p_drop:
        C = lambda site: ops.dropout_ctr_hi(offset, layer, site)
        masks = dict(pos=_mask(ops, (B, 2 * L, D), p_drop, seed, ops.dropout_ctr_hi(offset, 255, ops.SITE_POS)),
                     prob=_mask(ops, (B, n, L, L), p_drop, seed, C(ops.SITE_PROB)),
                     attn_out=_mask(ops, (B, L, D), p_drop, seed, C(ops.SITE_ATTN_OUT)),
                     ff_act=_mask(ops, (B, L, 4 * D), p_drop, seed, C(ops.SITE_FF_ACT)),
                     ff_out=_mask(ops, (B, L, D), p_drop, seed, C(ops.SITE_FF_OUT)))
        ref = O.xlnet_layer_dropout(hr, pr, n, 0.03, {k: m.double() for k, m in masks.items()}, p_drop)
    else:
        ref = O.xlnet_layer(hr, pr, n, 0.03)
    ref.backward(dout.double())
    close(runs[0][0], hr.grad.reshape(B * L, D).float(), rtol=1e-4, atol=3e-4 if p_drop else 2e-4)
    for k, gt in zip(ORDER, runs[0][1:]):
        close(gt.reshape(-1), pr[k].grad.reshape(-1).float(), rtol=1e-4, atol=8e-4 if p_drop else 5e-4,
              msg=lambda m, k=k: f"{k}: {m}")


@pytest.mark.parametrize("N,V,D,eps", [(37, 1001, 64, 0.0), (130, 5003, 128, 0.1)])
def test_gemm_softmax_grad_fused(ops, N, V, D, eps):
    """dX / dW of the head with the CE backward fused into the A operand == autograd."""
    g = torch.Generator().manual_seed(N + V)
    x = torch.randn(N, D, generator=g).requires_grad_()
    W = (0.3 * torch.randn(V, D, generator=g)).requires_grad_()
    y = torch.randint(0, V, (N,), generator=g)
    T = 0.7
    logits = (x @ W.t()) / T
    loss = torch.nn.functional.cross_entropy(logits, y, label_smoothing=eps)
    (loss * 1.3).backward()
    ld = ops.pad_ld(V)
    buf = torch.zeros(N, ld, device=DEV)
    buf[:, :V] = cu(logits.detach())
    lg = buf[:, :V]
    _, _, lse = ops.softmax_ce_fwd(lg, cu(y), V, eps)
    gout = torch.tensor(1.3, device=DEV)
    dx = ops.gemm_softmax_grad(lg, lse, cu(y), gout, V, cu(W.detach()), False, alpha=1 / T, label_smoothing=eps, splitk=-1)
    close(dx, x.grad, rtol=1e-4, atol=1e-6)
    dW = torch.ones(V, D, device=DEV)
    ops.gemm_softmax_grad(lg, lse, cu(y), gout, V, cu(x.detach()), True, alpha=1 / T, label_smoothing=eps, out=dW, accumulate=True)
    close(dW - 1, W.grad, rtol=1e-4, atol=2e-6)


# ------------------------------------------------------------------------------------ GPT-2 / BERT attention core
@pytest.mark.parametrize("B,L,D,n,causal,p", [(4, 20, 64, 4, True, 0.0), (3, 50, 128, 2, True, 0.0), (2, 100, 128, 2, False, 0.0),
                                              (3, 33, 64, 4, False, 0.1), (2, 21, 32, 2, True, 0.3), (2, 128, 32, 1, True, 0.0),
                                              (3, 33, 128, 4, False, 0.1), (2, 100, 512, 8, True, 0.2), (2, 65, 64, 2, False, 0.0),
                                              (5, 7, 64, 1, True, 0.0), (2, 96, 128, 2, False, 0.3),
                                              # beyond 128 positions / head widths without an LDS-kernel instance (general kernels,
                                              # csrc/xlnet_attn_long.hip): d_head 32, 64, 48, 8, 128, 24
                                              (2, 129, 64, 2, True, 0.0), (2, 200, 128, 2, False, 0.2), (3, 50, 96, 2, True, 0.1),
                                              (2, 33, 16, 2, False, 0.0), (2, 70, 256, 2, True, 0.3), (1040, 130, 24, 1, True, 0.0),
                                              (2, 20, 320, 2, True, 0.1), (2, 140, 256, 1, False, 0.0),
                                              (2, 30, 100, 4, True, 0.1), (2, 130, 36, 4, False, 0.0)])
def test_mha_fwd_bwd(ops, B, L, D, n, causal, p):
    g = torch.Generator().manual_seed(B + L + D + int(causal))
    dh = D // n
    seed, ctr = 5, ops.dropout_ctr_hi(3, 1, ops.SITE_PROB)
    qkv = torch.randn(B * L, 3 * D, generator=g)
    qkv_r = qkv.clone().requires_grad_()
    q, k, v = (qkv_r[:, i * D:(i + 1) * D].view(B, L, n, dh).transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) / dh ** 0.5
    if causal:
        s = s.masked_fill(~torch.tril(torch.ones(L, L, dtype=torch.bool)), float("-inf"))
    prob = torch.softmax(s, -1)
    if p > 0:
        prob = prob * _mask(ops, (B, n, L, L), p, seed, ctr) / (1 - p)
    ref = (prob @ v).transpose(1, 2).reshape(B * L, D)
    dout = torch.randn(B * L, D, generator=g)
    ref.backward(dout)
    dq = cu(qkv)
    drop = (p, seed, ctr) if p > 0 else ops.NO_DROP
    out, lse = ops.mha_fwd(dq[:, :D], dq[:, D:2 * D], dq[:, 2 * D:], B, L, n, causal, drop)
    close(out, ref.detach(), atol=3e-5)
    dqkv = ops.mha_bwd(dq[:, :D], dq[:, D:2 * D], dq[:, 2 * D:], out, lse, cu(dout), B, L, n, causal, drop, fused_out=True)
    close(dqkv, qkv_r.grad, rtol=1e-4, atol=2e-4)
    # separate (non-fused) operands
    a, b_, c = (cu(qkv[:, i * D:(i + 1) * D]) for i in range(3))
    out2, lse2 = ops.mha_fwd(a, b_, c, B, L, n, causal, drop)
    assert torch.equal(out2, out)
    g1, g2, g3 = ops.mha_bwd(a, b_, c, out2, lse2, cu(dout), B, L, n, causal, drop)
    close(torch.cat([g1, g2, g3], 1), qkv_r.grad, rtol=1e-4, atol=2e-4)


def test_gemm_resid_dropout_epilogue_and_pos_emb(ops):
    g = torch.Generator().manual_seed(12)
    M, N, K, p, seed, ctr = 150, 96, 64, 0.3, 2, ops.dropout_ctr_hi(1, 0, ops.SITE_FF_OUT)
    A, W, bias, R = (torch.randn(M, K, generator=g), torch.randn(K, N, generator=g), torch.randn(N, generator=g),
                     torch.randn(M, N, generator=g))
    m = _mask(ops, (M, N), p, seed, ctr)
    out = ops.gemm(cu(A), cu(W), bias=cu(bias), epilogue=ops.EPI_BIAS_RESID, aux=cu(R), drop=(p, seed, ctr))
    close(out, (A @ W + bias) * m / (1 - p) + R, atol=1e-4)
    out = ops.gemm(cu(A), cu(W), bias=cu(bias), epilogue=ops.EPI_BIAS_RESID, aux=cu(R))
    close(out, A @ W + bias + R, atol=1e-4)
    B, L, D = 37, 20, 64
    x, pos, tt = torch.randn(B, L, D, generator=g), torch.randn(L + 2, D, generator=g), torch.randn(2, D, generator=g)
    out = ops.add_pos_fwd(cu(x), cu(pos[:L]), cu(tt[0]))
    close(out, x + pos[:L] + tt[0], atol=1e-6)
    dpos = torch.zeros(L, D, device=DEV)
    dy = torch.randn(B, L, D, generator=g)
    ops.add_pos_bwd_(cu(dy), dpos)
    close(dpos, dy.sum(0), atol=1e-4)


# ------------------------------------------------------------------------------------------
# StochasticSwapNoise (t4r_swap_noise)
@pytest.mark.parametrize("name", ["xlnet_mlm_prepost_concat_train", "xlnet_mlm_prepost_sum_train"])
def test_swap_noise_replays_reference_draws(name):
    """every recorded augment() call of the reference (int64 ids and fp32 values), bit exact"""
    import golden_utils as gu
    from transformers4rec_amd import ops

    d = gu.load(name)
    ids = gu.t(d["in/item_id"]).to(DEV)
    n_calls = 0
    for k in d:
        if not k.startswith("draw/ssn_bern/"):
            continue
        _, _, mod, feat = k.split("/")
        x = gu.t(d["in/" + feat]).to(DEV)
        out = ops.swap_noise(x, ids, float(d["meta/ssn_p"]), 0, gu.t(d[k]).to(DEV),
                             gu.t(d[f"draw/ssn_perm/{mod}/{feat}"]).to(DEV))
        assert torch.equal(out.cpu(), gu.t(d[f"out/ssn/{mod}/{feat}"])), (mod, feat)
        n_calls += 1
    assert n_calls >= 6


@pytest.mark.parametrize("p", [0.1, 0.3, 0.5, 0.7])
def test_swap_noise_device_draws_properties(p):
    """mirrors tests/unit/torch/tabular/test_transformations.py:29-56 (replacement rate within 0.15 of
    replacement_prob on the non-padded positions) and adds what the algorithm guarantees: padding is
    never touched, replacements are drawn WITHOUT replacement from the non-padded values."""
    from transformers4rec_amd import ops

    B, L = 100, 80
    g = torch.Generator().manual_seed(0)
    ids = torch.tril(torch.randint(1, 100, (B, L), generator=g), 1)
    uniq = (torch.arange(B * L).view(B, L) + 1) * (ids != 0)          # distinct non-pad values
    cont = torch.tril(torch.rand((B, L), generator=g), 1)
    per_session = torch.randint(1, 100, (B,), generator=g)
    for x in (ids, uniq, cont, per_session):
        out = ops.swap_noise(x.to(DEV), ids.to(DEV), p, 0, seed=7, ctr_hi=11).cpu()
        mask = (ids != 0) if x.ndim == 2 else (ids[:, 0] != 0)
        assert torch.equal(out[~mask], x[~mask])                       # padding untouched
        if x is uniq:
            changed = (out != x) & mask
            rate = changed.float().sum() / mask.float().sum()
            assert abs(float(rate) - p) < 0.05
            src = out[changed]
            assert src.unique().numel() == src.numel()                 # sampled without replacement
            assert bool(torch.isin(src, x[mask]).all())                # ... from the non-pad values
        elif x.ndim == 2:
            rate = ((out != x) & mask).float().sum() / mask.float().sum()
            assert abs(float(rate) - p) < 0.15
        assert bool(torch.isin(out[mask], x[mask]).all())
    # a different stream position gives a different draw; the same one reproduces
    a = ops.swap_noise(uniq.to(DEV), ids.to(DEV), p, 0, seed=7, ctr_hi=11)
    b = ops.swap_noise(uniq.to(DEV), ids.to(DEV), p, 0, seed=7, ctr_hi=11)
    c = ops.swap_noise(uniq.to(DEV), ids.to(DEV), p, 0, seed=7, ctr_hi=12)
    assert torch.equal(a, b) and not torch.equal(a, c)


def test_swap_noise_edge_cases():
    from transformers4rec_amd import ops

    ids = torch.zeros((4, 6), dtype=torch.int64, device=DEV)          # all padding: nothing to swap
    x = torch.arange(24, device=DEV).view(4, 6)
    assert torch.equal(ops.swap_noise(x, ids, 0.9), x)
    ids[0, 0] = 5                                                     # one valid value: swaps with itself
    assert torch.equal(ops.swap_noise(x, ids, 1.0), x)
    ids = torch.ones((3, 5), dtype=torch.int64, device=DEV)
    xf = torch.rand((3, 5), device=DEV)
    assert torch.equal(ops.swap_noise(xf, ids, 0.0), xf)              # p = 0: identity
    out = ops.swap_noise(xf, ids, 1.0, seed=1)                        # p = 1: a permutation of the values
    assert torch.equal(out.flatten().sort().values, xf.flatten().sort().values)
    e = torch.empty((0, 5), dtype=torch.int64, device=DEV)
    assert ops.swap_noise(e, e, 0.5).shape == (0, 5)


# ------------------------------------------------------------------------------------------
# fused eval head: rank of the target without materialising the scores
@pytest.mark.parametrize("N,V,D", [(1, 5, 8), (70, 1000, 32), (257, 4099, 128), (1500, 333, 64)])
def test_rank_of_target_matches_topk_and_sort(N, V, D):
    from transformers4rec_amd import ops

    g = torch.Generator().manual_seed(N + V)
    x = torch.randn((N, D), generator=g)
    W = torch.randn((V, D), generator=g)
    if V > 10:                       # exact ties: duplicated item rows (same score for two columns)
        W[7] = W[3]
        W[V - 1] = W[V // 2]
    y = torch.randint(0, V, (N,), generator=g)
    if V > 10:
        y[0], y[N // 2] = 7, V // 2   # targets inside a tie group: the lower index ranks first
    xd, Wd, yd = x.to(DEV), W.to(DEV), y.to(DEV)
    ranks = ops.rank_of_target(xd, Wd, yd, alpha=0.5).cpu()
    scores = ops.gemm(xd, Wd, False, True, alpha=0.5).cpu()          # the same kernel's scores
    t = scores[torch.arange(N), y]
    idx = torch.arange(V)[None]
    ref = ((scores > t[:, None]) | ((scores == t[:, None]) & (idx < y[:, None]))).sum(1).to(torch.int32)
    assert torch.equal(ranks, ref)
    if V > 10:
        assert int(ranks[0]) >= 1 and scores[0, 3] == scores[0, 7]   # column 3 ties with the target 7 and precedes it
    k = min(20, V)
    _, topi = ops.topk(scores.to(DEV), k, V)
    hit = (topi.cpu() == y[:, None])
    assert torch.equal(hit.any(1), ranks < k)
    assert torch.equal(hit.float().argmax(1)[hit.any(1)].to(torch.int32), ranks[ranks < k])


def test_topk_ties_and_fallback_path(ops):
    """ties resolve to the lower index; rows with more than TOPK_CAP values at the threshold
    (constant rows, heavy duplicates) take the sorted-list fallback and must agree"""
    V, k = 5000, 10
    s = torch.zeros(4, V)
    s[1, 100:3000] = 1.0                                      # 2900 equal maxima -> candidate overflow
    s[2] = torch.arange(V).float() % 7                       # many duplicates of the top value
    s[3] = -torch.arange(V).float()                          # strictly decreasing: top-k = first k
    v, i = ops.topk(cu(s), k)
    order = torch.argsort(-s, dim=1, stable=True)[:, :k]      # value desc, index asc
    assert torch.equal(i.cpu(), order)
    assert torch.equal(v.cpu(), torch.gather(s, 1, order))
    # padded leading dimension + V not a multiple of 4 + k = 64
    g = torch.Generator().manual_seed(0)
    s2 = torch.randn(3, 1003, generator=g)
    buf = torch.full((3, 1024), 9e9)
    buf[:, :1003] = s2
    v2, i2 = ops.topk(cu(buf)[:, :1003], 64, 1003)
    rv, ri = torch.topk(s2, 64, dim=-1)
    assert torch.equal(v2.cpu(), rv) and torch.equal(i2.cpu(), ri)
    # 64 < k <= 256 on the same adversarial rows: the selection fallback (no LDS lists of that size)
    k = 100
    v3, i3 = ops.topk(cu(s), k)
    order = torch.argsort(-s, dim=1, stable=True)[:, :k]
    assert torch.equal(i3.cpu(), order)
    assert torch.equal(v3.cpu(), torch.gather(s, 1, order))


# ------------------------------------------------------------------------------------ deterministic table gradient
@pytest.mark.parametrize("n,rows,dim,W,col,ids_div", [
    (1, 10, 8, 8, 0, 1), (17, 5, 64, 64, 0, 1), (1000, 300, 128, 128, 0, 1), (20480, 100001, 128, 128, 0, 1),
    (40000, 11, 64, 200, 72, 1),        # hot rows: every segment spans many super-chunks
    (5000, 41, 200, 336, 100, 1),       # odd width inside a concatenated row
    (3000, 1000, 512, 512, 0, 1), (700, 50, 600, 600, 0, 1),      # wide rows: second column block
    (256, 17, 32, 40, 8, 20),           # per-session feature: gradient summed over the L = 20 positions
    (300000, 1000, 64, 64, 0, 1),       # S > 1 super-chunks
])
def test_embedding_bwd_sorted_is_exact_and_deterministic(ops, n, rows, dim, W, col, ids_div):
    """sort + segmented sum == index_add of the oracle (fp64 accumulation as the referee), padding and
    out-of-range ids carry no gradient, two runs are bit-identical (no atomics)."""
    g = torch.Generator().manual_seed(n + rows)
    ids = torch.randint(0, rows, (n,), generator=g)          # includes padding id 0
    if n > 4:
        ids[3] = rows + 5                                    # out of range: ignored
        ids[-1] = ids[0]
    dout = torch.randn(n * ids_div, W, generator=g)
    keys, perm = ops.sort_ids(cu(ids), rows, 0)
    kc, pc = keys.cpu().long(), perm.cpu().long()
    valid = (ids != 0) & (ids < rows)
    want_keys = torch.where(valid, ids, torch.full_like(ids, rows))
    assert torch.equal(kc, want_keys.sort(stable=True).values)
    assert torch.equal(pc, want_keys.sort(stable=True).indices)       # stable: ascending lookup order within a row
    grows = dout.view(n, ids_div, W)[:, :, col: col + dim].double().sum(1)
    ref = torch.zeros(rows, dim, dtype=torch.float64).index_add_(0, ids[valid], grows[valid])
    base = torch.randn(rows, dim, generator=g)
    outs = []
    for _ in range(2):
        dt = cu(base).clone()
        ops.embedding_bwd_sorted(cu(dout), keys, perm, dt, col, dim, ids_div)
        outs.append(dt.cpu())
    assert torch.equal(outs[0], outs[1]), "two runs differ: the scatter is not deterministic"
    err = (outs[0].double() - base.double() - ref).abs().max()
    scale = max(1.0, float(ref.abs().max()))
    assert float(err) <= 2e-6 * scale * max(1, (n // rows) ** 0.5), float(err)
    assert torch.equal(outs[0][0], base[0]), "the padding row received gradient"


# ------------------------------------------------------------------------------------ non-materialising head
@pytest.mark.parametrize("N,V,D,eps,chunk", [(37, 1001, 64, 0.0, 256), (130, 5003, 128, 0.1, 1024),
                                              (64, 3000, 32, 0.0, None), (5, 777, 16, 0.2, 64)])
def test_linear_softmax_ce_fused_fwd_bwd(ops, N, V, D, eps, chunk):
    """chunk-streamed linear + softmax-CE (no [N, V] tensor) == torch autograd of F.cross_entropy(x @ W^T / T),
    including label smoothing, temperature, labels in the first / last chunk and a ragged last chunk."""
    g = torch.Generator().manual_seed(N * 7 + V)
    x = torch.randn(N, D, generator=g).requires_grad_()
    W = (0.3 * torch.randn(V, D, generator=g)).requires_grad_()
    y = torch.randint(0, V, (N,), generator=g)
    y[0], y[-1] = 0, V - 1
    T = 0.7
    loss = torch.nn.functional.cross_entropy((x @ W.t()) / T, y, label_smoothing=eps)
    (loss * 1.3).backward()
    lh, rows, lse = ops.linear_softmax_ce_fwd(cu(x.detach()), cu(W.detach()), cu(y), 1 / T, eps, chunk_cols=chunk)
    assert abs(float(lh) - float(loss)) < 2e-6 * max(1.0, abs(float(loss)))
    close(lse, torch.logsumexp((x @ W.t()).detach() / T, 1), rtol=1e-6, atol=2e-6)
    close(rows.mean(), loss.detach(), rtol=1e-6, atol=2e-6)
    dW = torch.ones(V, D, device=DEV)
    dx = ops.linear_softmax_ce_bwd(cu(x.detach()), cu(W.detach()), cu(y), lse, torch.tensor(1.3, device=DEV), dW=dW,
                                   alpha=1 / T, label_smoothing=eps, chunk_cols=chunk)
    close(dx, x.grad, rtol=1e-4, atol=1e-6)
    close(dW - 1, W.grad, rtol=1e-4, atol=2e-6)
    # same bits as the materialised pipeline's statistics (the chunks come from the same GEMM)
    logits = ops.gemm(cu(x.detach()), cu(W.detach()), False, True, alpha=1 / T, ldc=ops.pad_ld(V))
    _, _, lse_m = ops.softmax_ce_fwd(logits, cu(y), V, eps)
    close(lse, lse_m, rtol=0, atol=2e-6)


# ------------------------------------------------------------------------------------ bf16 / fp16 matrix-core GEMM variants
def _round_to(x, mode):
    if mode == "bf16":
        return x.to(torch.bfloat16).float()
    if mode == "fp16":
        return x.to(torch.float16).float()
    return x


@pytest.mark.parametrize("mode", ["fp32_bf16x3", "bf16", "fp16"])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(128, 128, 128), (76, 132, 36), (300, 64, 512), (36, 1004, 128), (4, 8, 4),
                                   (260, 384, 100), (1024, 260, 64)])
def test_gemm_precision_modes_layouts(ops, mode, ta, tb, M, N, K):
    """the bf16 / fp16 matrix-core variants of the GEMM in every layout (dims multiples of 4: 16-byte loadable):
    fp32_bf16x3 must meet the fp32 kernel's tolerance; the mixed-precision modes must equal the product of the
    ROUNDED operands accumulated in fp32 (that is their definition), which is also close to the fp32 product."""
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K + ta * 2 + tb)
    A = torch.randn((K, M) if ta else (M, K), generator=g)
    B = torch.randn((N, K) if tb else (K, N), generator=g)
    Ar, Br = _round_to(A, mode), _round_to(B, mode)
    ref = (Ar.t() if ta else Ar).double() @ (Br.t() if tb else Br).double()
    before = ops.get_precision()
    with ops.precision(mode):
        assert ops.get_precision() == mode
        out = ops.gemm(cu(A), cu(B), bool(ta), bool(tb), alpha=0.5)
    assert ops.get_precision() == before            # the default is "auto" unless T4R_GEMM_PREC says otherwise
    close(out, (0.5 * ref).float(), rtol=1e-5, atol=1e-4)
    if mode != "fp32_bf16x3":     # and the rounding itself costs what half precision costs, no more
        full = (A.t() if ta else A).double() @ (B.t() if tb else B).double()
        tol = (2 ** -8 if mode == "bf16" else 2 ** -11) * 4 * (K ** 0.5)
        assert float((out.cpu().double() - 0.5 * full).abs().max()) < tol


@pytest.mark.parametrize("mode", ["fp32_bf16x3", "bf16", "fp16"])
def test_gemm_precision_modes_features(ops, mode):
    """epilogues, split-K, accumulate, batch stride, the 128 x 128 tile and the softmax-gradient A operand"""
    g = torch.Generator().manual_seed(11)
    rnd = lambda x: _round_to(x, mode)
    tol = dict(rtol=1e-4, atol=2e-4)
    with ops.precision(mode):
        M, N, K = 200, 192, 96
        A, W, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g)
        pre = rnd(A) @ rnd(W).t() + bias
        aux = torch.empty((M, N), device=DEV)
        out = ops.gemm(cu(A), cu(W), False, True, bias=cu(bias), epilogue=ops.EPI_BIAS_GELU, aux=aux)
        close(aux, pre, **tol)
        close(out, torch.nn.functional.gelu(pre), **tol)
        close(ops.gemm(cu(A), cu(W), False, True, bias=cu(bias), epilogue=ops.EPI_BIAS_RELU), torch.relu(pre), **tol)
        res = torch.randn(M, N, generator=g)
        close(ops.gemm(cu(A), cu(W), False, True, bias=cu(bias), epilogue=ops.EPI_BIAS_RESID, aux=cu(res)), pre + res, **tol)
        # split-K wgrad shape (TN, long K), overwrite / accumulate
        K2 = 5000
        A2, B2 = torch.randn(K2, 72, generator=g), torch.randn(K2, 92, generator=g)
        ref = (rnd(A2).t().double() @ rnd(B2).double()).float()
        close(ops.gemm(cu(A2), cu(B2), True, False, splitk=-1), ref, rtol=1e-4, atol=2e-3)
        acc = cu(torch.ones(72, 92))
        ops.gemm(cu(A2), cu(B2), True, False, splitk=-1, accumulate=True, out=acc)
        close(acc, ref + 1, rtol=1e-4, atol=2e-3)
        # large plain NT product: the one-plane precisions take the 128 x 128 tile here
        X, Wv = torch.randn(1100, 64, generator=g), torch.randn(40004, 64, generator=g)
        out = ops.gemm(cu(X), cu(Wv), False, True, alpha=1 / 0.7, ldc=ops.pad_ld(40004))
        close(out, (rnd(X) @ rnd(Wv).t()) / 0.7, **tol)
        # the head's backward products with the softmax gradient formed in the A operand
        Nr, V, D = 130, 5004, 128
        x = torch.randn(Nr, D, generator=g)
        Wt = 0.3 * torch.randn(V, D, generator=g)
        y = torch.randint(0, V, (Nr,), generator=g)
        logits = x @ Wt.t()
        buf = torch.zeros(Nr, ops.pad_ld(V), device=DEV)
        buf[:, :V] = cu(logits)
        lg = buf[:, :V]
    _, _, lse = ops.softmax_ce_fwd(lg, cu(y), V, 0.0)
    dl = (torch.softmax(logits, 1) - torch.nn.functional.one_hot(y, V)) / Nr
    with ops.precision(mode):
        dx = ops.gemm_softmax_grad(lg, lse, cu(y), None, V, cu(Wt), False, splitk=-1)
        dW = torch.zeros(V, D, device=DEV)
        ops.gemm_softmax_grad(lg, lse, cu(y), None, V, cu(x), True, out=dW, accumulate=True)
    loose = dict(rtol=2e-2, atol=2e-5) if mode != "fp32_bf16x3" else dict(rtol=1e-4, atol=2e-6)
    close(dx, dl @ Wt, **loose)
    close(dW, dl.t() @ x, **loose)


# ------------------------------------------------------------------------------------ opt-in attention padding mask
@pytest.mark.parametrize("B,L,D,n", [(6, 20, 128, 4), (5, 20, 64, 4), (4, 40, 64, 4), (3, 9, 32, 4), (4, 32, 64, 2)])
def test_xlnet_attention_padding_mask(ops, B, L, D, n):
    """key_len (opt-in, default off): keys >= key_len[b] masked except on the diagonal, forward and backward of the
    whole layer on both kernel families (matrix-core: L <= 32 and d_head 16 / 32; VALU otherwise) vs the oracle,
    whose mask is pinned against HF XLNetModel(attention_mask=...) in tests/test_oracle_vs_hf.py."""
    g = torch.Generator().manual_seed(B * 5 + L + D)
    prm = _layer_params(g, D, n)
    pr = {k: v.clone().requires_grad_() for k, v in prm.items()}
    h = torch.randn(B, L, D, generator=g)
    hr = h.clone().requires_grad_()
    key_len = torch.randint(1, L + 1, (B,), generator=g).to(torch.int32)
    key_len[0], key_len[-1] = L, 1
    ref = O.xlnet_layer(hr, pr, n, 0.03, key_len=key_len)
    dout = torch.randn(B, L, D, generator=g)
    ref.backward(dout)
    pos = cu(O.xlnet_pos_emb(L, D))
    params = [cu(prm[k]) for k in ORDER]
    out, ws = ops.xlnet_layer_fwd(cu(h).view(B * L, D), pos, params, B, L, n, 0.03, key_len=cu(key_len))
    close(out, ref.detach().reshape(B * L, D), atol=5e-5)
    plain, _ = ops.xlnet_layer_fwd(cu(h).view(B * L, D), pos, params, B, L, n, 0.03)
    assert float((plain - out).abs().max()) > 1e-4          # and None keeps the reference's unmasked attention
    grads = [torch.zeros_like(t) for t in params]
    dh = ops.xlnet_layer_bwd(cu(h).view(B * L, D), pos, params, grads, ws, cu(dout).view(B * L, D), B, L, n, 0.03,
                             key_len=cu(key_len))
    close(dh, hr.grad.reshape(B * L, D), rtol=1e-4, atol=3e-4)
    for k, gt in zip(ORDER, grads):
        close(gt.reshape(-1), pr[k].grad.reshape(-1), rtol=1e-4, atol=8e-4, msg=lambda mm, k=k: f"{k}: {mm}")
    # session_lengths: non-pad count (+ the MLM inference slot)
    ids = (torch.arange(L)[None] < key_len[:, None]).long() * 7
    assert torch.equal(ops.session_lengths(cu(ids)).cpu(), key_len)
    assert torch.equal(ops.session_lengths(cu(ids), 0, 1).cpu(), key_len + 1)


@pytest.mark.parametrize("B,L,D,n,causal,p", [(4, 20, 64, 2, True, 0.0), (3, 50, 128, 2, True, 0.0), (4, 100, 128, 2, False, 0.0),
                                              (3, 33, 32, 2, False, 0.0), (3, 21, 64, 2, True, 0.2), (4, 96, 256, 4, False, 0.1),
                                              (3, 150, 64, 2, True, 0.1), (3, 140, 96, 2, False, 0.0)])
def test_mha_padding_mask(ops, B, L, D, n, causal, p):
    """opt-in key padding mask of the GPT-2 / BERT attention core (both kernel families) vs the oracle's sdpa,
    whose mask is pinned against HF in tests/test_oracle_vs_hf.py; None keeps the unmasked reference behaviour."""
    g = torch.Generator().manual_seed(B + L + D + int(causal))
    dh = D // n
    seed, ctr = 5, ops.dropout_ctr_hi(3, 1, ops.SITE_PROB)
    key_len = torch.randint(1, L + 1, (B,), generator=g).to(torch.int32)
    key_len[0], key_len[-1] = L, 1
    qkv = torch.randn(B * L, 3 * D, generator=g)
    qkv_r = qkv.clone().requires_grad_()
    q, k, v = (qkv_r[:, i * D:(i + 1) * D].view(B, L, n, dh).transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) / dh ** 0.5
    if causal:
        s = s.masked_fill(~torch.tril(torch.ones(L, L, dtype=torch.bool)), float("-inf"))
    s = s.masked_fill(torch.arange(L)[None, None, None, :] >= key_len.reshape(-1, 1, 1, 1).long(), float("-inf"))
    prob = torch.softmax(s, -1)
    if p > 0:
        prob = prob * _mask(ops, (B, n, L, L), p, seed, ctr) / (1 - p)
    ref = (prob @ v).transpose(1, 2).reshape(B * L, D)
    dout = torch.randn(B * L, D, generator=g)
    ref.backward(dout)
    dq = cu(qkv)
    drop = (p, seed, ctr) if p > 0 else ops.NO_DROP
    kl = cu(key_len)
    out, lse = ops.mha_fwd(dq[:, :D], dq[:, D:2 * D], dq[:, 2 * D:], B, L, n, causal, drop, key_len=kl)
    close(out, ref.detach(), atol=3e-5)
    dqkv = ops.mha_bwd(dq[:, :D], dq[:, D:2 * D], dq[:, 2 * D:], out, lse, cu(dout), B, L, n, causal, drop, fused_out=True,
                       key_len=kl)
    close(dqkv, qkv_r.grad, rtol=1e-4, atol=2e-4)
    plain, _ = ops.mha_fwd(dq[:, :D], dq[:, D:2 * D], dq[:, 2 * D:], B, L, n, causal, drop)
    assert float((plain - out).abs().max()) > 1e-4


def test_fp16_softmax_gradient_is_scaled_into_range(ops):
    """fp16 mode, large vocabulary: (1/N) (softmax - onehot) ~ 1e-9 underflows fp16 (smallest subnormal 6e-8); the
    operand is scaled by a power of two before rounding and alpha undoes it (the reference's GradScaler, per launch)."""
    g = torch.Generator().manual_seed(3)
    N, V, D = 3000, 40000, 64
    x = torch.randn(N, D, generator=g)
    W = 0.05 * torch.randn(V, D, generator=g)
    y = torch.randint(0, V, (N,), generator=g)
    logits = x @ W.t()
    dl = (torch.softmax(logits, 1) - torch.nn.functional.one_hot(y, V)) / N
    assert float(dl.abs().median()) < 6e-8                       # most entries are below fp16's range unscaled
    buf = torch.zeros(N, ops.pad_ld(V), device=DEV)
    buf[:, :V] = cu(logits)
    lg = buf[:, :V]
    _, _, lse = ops.softmax_ce_fwd(lg, cu(y), V, 0.0)
    with ops.precision("fp16"):
        dx = ops.gemm_softmax_grad(lg, lse, cu(y), None, V, cu(W), False, splitk=-1)
        dW = torch.zeros(V, D, device=DEV)
        ops.gemm_softmax_grad(lg, lse, cu(y), None, V, cu(x), True, out=dW, accumulate=True)
    ref_dx, ref_dW = dl @ W, dl.t() @ x
    # half-precision tolerance relative to the largest entry; an unscaled fp16 operand loses the whole softmax term
    assert float((dx.cpu() - ref_dx).abs().max()) < 4e-3 * float(ref_dx.abs().max())
    assert float((dW.cpu() - ref_dW).abs().max()) < 4e-3 * float(ref_dW.abs().max())
    nolabel = torch.ones(V, dtype=torch.bool)
    nolabel[y] = False                                            # rows that only see the softmax term
    assert float((dW.cpu()[nolabel] - ref_dW[nolabel]).abs().max()) < 2e-2 * float(ref_dW[nolabel].abs().max())


def test_log_uniform_device_sampler_matches_the_reference_distribution(ops):
    """the closed-form inverse-CDF sampler draws from exactly LogUniformSampler.dist (prediction_task.py:766-786):
    range, zero mass below min_id, and bin frequencies of 400 k draws against the distribution's own bin masses."""
    import transformers4rec_amd as tr

    V, min_id, n = 100_001, 1, 400_000
    s = tr.LogUniformSampler(max_n_samples=100, max_id=V, min_id=min_id)
    ids = ops.log_uniform_sample(n, min_id, V, 1234, 7, DEV).cpu()
    assert int(ids.min()) >= min_id and int(ids.max()) < V
    edges = torch.unique(torch.logspace(0, 5, 26).long().clamp_(min_id, V))
    cdf = torch.cat([torch.zeros(1, dtype=torch.float64), s.dist.double().cumsum(0)])
    for lo, hi in zip(edges[:-1].tolist(), edges[1:].tolist()):
        want = float(cdf[hi] - cdf[lo]) * n
        got = int(((ids >= lo) & (ids < hi)).sum())
        assert abs(got - want) < 5 * (want ** 0.5) + 5, (lo, hi, got, want)
    # another stream position gives other draws; the same position repeats
    again = ops.log_uniform_sample(1000, min_id, V, 1234, 7, DEV).cpu()
    other = ops.log_uniform_sample(1000, min_id, V, 1234, 8, DEV).cpu()
    assert torch.equal(again, ids[:1000]) and not torch.equal(other, again)
    # the module: unique, sorted, truncated, on the labels' device -- as the reference's sample()
    s.to(DEV)
    neg = s.sample(torch.ones(3, dtype=torch.long, device=DEV))
    assert neg.device.type == "cuda" and neg.numel() <= 100 and bool((neg[1:] > neg[:-1]).all())
    s.device_sampler = False
    neg2 = s.sample(torch.ones(3, dtype=torch.long, device=DEV))
    assert neg2.numel() <= 100 and int(neg2.min()) >= min_id


# ------------------------------------------------------------------------------------------
# materialised head for d_model <= 128 (csrc/head_split.hip)
def _head_reference(x, W, labels, alpha, smooth, gout, logits, yoff=0, V=None):
    """fp64: logits, and the two backward products formed from the GIVEN fp32 logits (the kernels' input)"""
    N, Vc = logits.shape
    V = Vc if V is None else V
    lg = alpha * (x.double() @ W.double().t())
    return lg


@pytest.mark.parametrize("N,V,D,alpha,smooth", [(77, 1000, 64, 1.0, 0.0), (33, 257, 32, 1.0, 0.0), (130, 999, 96, 2.0, 0.0),
                                                 (200, 5000, 128, 0.5, 0.1), (1, 40, 128, 1.0, 0.0)])
def test_head_split_products_match_fp64(ops, N, V, D, alpha, smooth):
    """logits, d X, d W of the hoisted-cut head against fp64 (errors at the level of the fp32 matrix-core path,
    transformers4rec/torch/model/prediction_task.py:664 + autograd through CrossEntropyLoss :446)"""
    g = torch.Generator(device=DEV).manual_seed(N)
    x = torch.randn(N, D, device=DEV, generator=g)
    W = torch.randn(V, D, device=DEV, generator=g) * 0.3
    labels = torch.randint(0, V, (N,), device=DEV, generator=g)
    gout = torch.tensor(1.7, device=DEV)
    ws = ops.head_split_prepare(x, V)
    logits = ops.head_split_logits(ws, x, W, alpha=alpha, ldc=ops.pad_ld(V))
    lg64 = alpha * (x.double() @ W.double().t())
    assert float((logits.double() - lg64).abs().max()) < 2e-6 * float(lg64.abs().max())
    loss, rows, lse = ops.softmax_ce_fwd(logits, labels, V, smooth)
    # the one-pass form: same logits (to rounding), statistics merged from the per-tile partials
    lg2, loss2, rows2, lse2 = ops.head_split_logits_ce(ws, x, W, labels, alpha=alpha, label_smoothing=smooth, ldc=ops.pad_ld(V))
    close(lg2, logits, rtol=0, atol=4e-6 * float(lg64.abs().max()))
    ref_rows = torch.nn.functional.cross_entropy(lg2.double(), labels, reduction="none", label_smoothing=smooth)
    assert float((rows2.double() - ref_rows).abs().max()) < 1e-5
    assert float((lse2.double() - torch.logsumexp(lg2.double(), 1)).abs().max()) < 1e-5
    assert abs(float(loss2) - float(ref_rows.mean())) < 1e-5
    p = torch.softmax(logits.double(), dim=1)
    onehot = torch.zeros_like(p)
    onehot[torch.arange(N, device=DEV), labels] = 1.0
    G = (1.7 / N) * (p - (1 - smooth) * onehot - smooth / V)
    dX64, dW64 = alpha * (G @ W.double()), alpha * (G.t() @ x.double())
    dX = ops.head_split_dx(ws, logits, lse, labels, gout, V, W, alpha=alpha, label_smoothing=smooth)
    dW0 = torch.randn(V, D, device=DEV, generator=g) * float(dW64.abs().max())
    dW = dW0.clone()
    ops.head_split_dw(ws, logits, lse, labels, gout, V, D, dW, alpha=alpha, label_smoothing=smooth, accumulate=True)
    dWn = torch.full((V, D), float("nan"), device=DEV)
    ops.head_split_dw(ws, logits, lse, labels, gout, V, D, dWn, alpha=alpha, label_smoothing=smooth, accumulate=False)
    assert float((dX.double() - dX64).abs().max()) < 5e-6 * float(dX64.abs().max())
    assert float((dWn.double() - dW64).abs().max()) < 5e-6 * float(dW64.abs().max())
    assert float((dW.double() - dW0.double() - dW64).abs().max()) < 1e-5 * float(dW64.abs().max())
    # no atomics anywhere: a second run gives the same bits
    dX2 = ops.head_split_dx(ws, logits, lse, labels, gout, V, W, alpha=alpha, label_smoothing=smooth)
    dW2 = torch.empty_like(dWn)
    ops.head_split_dw(ws, logits, lse, labels, gout, V, D, dW2, alpha=alpha, label_smoothing=smooth, accumulate=False)
    assert torch.equal(dX, dX2) and torch.equal(dWn, dW2)
    # agreement with the general path it replaces
    with ops.precision("fp32"):
        dX_g = ops.gemm_softmax_grad(logits, lse, labels, gout, V, W, False, alpha=alpha, label_smoothing=smooth, splitk=-1)
    close(dX, dX_g, rtol=1e-4, atol=1e-5 * float(dX64.abs().max()))


@pytest.mark.parametrize("sx,sw,gout", [(1.0, 1.0, 1.0), (3e-13, 2e7, 1.0), (5e11, 7e-9, 1.0), (1.0, 1.0, 3e-21), (40.0, 0.01, 6e9)])
def test_head_split_fp16_split_is_scale_free(ops, sx, sw, gout):
    """The forward and d X products run on a two-way fp16 split whose pieces only cover [6e-8, 65504]: power-of-two scales
    taken from max |X|, max |W| and g / N (csrc/head_split.hip: scale_of, mfma_split) position every tensor first.  The
    error against fp64, relative to the largest output, must not depend on the magnitudes of the inputs or of the
    upstream gradient -- fp16 range never shows through."""
    N, V, D = 150, 3000, 128
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(N, D, device=DEV, generator=g) * sx
    W = torch.randn(V, D, device=DEV, generator=g) * sw
    alpha = 1.0 / (sx * sw * 8.0)                      # logits of order one whatever the operand magnitudes
    labels = torch.randint(0, V, (N,), device=DEV, generator=g)
    ws = ops.head_split_prepare(x, V)
    logits, loss, rows, lse = ops.head_split_logits_ce(ws, x, W, labels, alpha=alpha, ldc=ops.pad_ld(V))
    lg64 = alpha * (x.double() @ W.double().t())
    assert torch.isfinite(logits).all()
    assert float((logits.double() - lg64).abs().max()) < 2e-6 * float(lg64.abs().max())
    go = torch.tensor(gout, device=DEV)
    dX = ops.head_split_dx(ws, logits, lse, labels, go, V, W, alpha=alpha)
    p = torch.softmax(logits.double(), dim=1)
    p[torch.arange(N, device=DEV), labels] -= 1.0
    dX64 = alpha * ((gout / N) * p) @ W.double()
    assert torch.isfinite(dX).all()
    assert float((dX.double() - dX64).abs().max()) < 5e-6 * float(dX64.abs().max())


def test_head_split_fp16_split_zero_operand(ops):
    """an all-zero operand (max |X| = 0: no scale to take) gives exact zeros, not NaN"""
    N, V, D = 40, 700, 64
    x = torch.zeros(N, D, device=DEV)
    W = torch.randn(V, D, device=DEV)
    labels = torch.randint(0, V, (N,), device=DEV)
    ws = ops.head_split_prepare(x, V)
    logits, loss, rows, lse = ops.head_split_logits_ce(ws, x, W, labels, ldc=ops.pad_ld(V))
    assert torch.equal(logits, torch.zeros_like(logits))
    assert abs(float(loss) - float(torch.log(torch.tensor(float(V))))) < 1e-5


def test_head_split_vocabulary_chunk(ops):
    """logits holding only the columns [yoff, yoff + Vc) of the problem (the chunk-streamed form): labels outside the
    chunk contribute only their softmax mass, eps / V and 1 / N refer to the full problem"""
    N, V, D, yoff, Vc = 50, 900, 64, 256, 300
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(N, D, device=DEV, generator=g)
    W = torch.randn(V, D, device=DEV, generator=g) * 0.3
    labels = torch.randint(0, V, (N,), device=DEV, generator=g)
    ws = ops.head_split_prepare(x, V)
    full = ops.head_split_logits(ws, x, W, ldc=ops.pad_ld(V))
    _, _, lse = ops.softmax_ce_fwd(full, labels, V, 0.1)
    chunk = torch.empty((N, ops.pad_ld(Vc)), device=DEV)[:, :Vc]
    chunk.copy_(full[:, yoff:yoff + Vc])
    p = torch.exp(full.double() - lse.double()[:, None])
    onehot = torch.zeros_like(p)
    onehot[torch.arange(N, device=DEV), labels] = 1.0
    G = ((p - 0.9 * onehot - 0.1 / V) / N)[:, yoff:yoff + Vc]
    dX = ops.head_split_dx(ws, chunk, lse, labels, None, V, W[yoff:yoff + Vc], label_smoothing=0.1, yoff=yoff)
    dW = torch.zeros(Vc, D, device=DEV)
    ops.head_split_dw(ws, chunk, lse, labels, None, V, D, dW, label_smoothing=0.1, accumulate=False, yoff=yoff)
    close(dX, (G @ W[yoff:yoff + Vc].double()).float(), rtol=1e-4, atol=1e-7)
    close(dW, (G.t() @ x.double()).float(), rtol=1e-4, atol=1e-7)


# ------------------------------------------------------------------------------------------
# token-stationary GEMM of the transformer body (csrc/tok_gemm.hip)
@pytest.mark.parametrize("M,N,K,tb", [(640, 128, 128, True), (640, 128, 128, False), (1000, 512, 128, True),
                                      (777, 128, 512, True), (640, 512, 128, False), (530, 128, 512, False),
                                      (600, 96, 64, True), (512, 64, 256, False), (1500, 32, 32, True)])
def test_tok_gemm_matches_fp64(ops, M, N, K, tb):
    """tokens x small weight in the default (fp32-accurate) mode goes through the token-stationary kernel: every
    supported width / orientation against fp64, at the accuracy of the fp32 matrix-core path"""
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    A = torch.randn(M, K, device=DEV, generator=g)
    B = torch.randn((N, K) if tb else (K, N), device=DEV, generator=g) * 0.2
    ref = A.double() @ (B.double().t() if tb else B.double())
    with ops.tok_gemm_min_rows(512):
        _tok_gemm_checks(ops, A, B, tb, ref, M, N, g)


def _tok_gemm_checks(ops, A, B, tb, ref, M, N, g):
    out = ops.gemm(A, B, False, tb, alpha=0.7)
    with ops.precision("fp32"):
        gen = ops.gemm(A, B, False, tb, alpha=0.7)
    scale = float(ref.abs().max())
    e_new, e_gen = float((out.double() - 0.7 * ref).abs().max()) / scale, float((gen.double() - 0.7 * ref).abs().max()) / scale
    assert e_new < max(2e-6, 3 * e_gen), (e_new, e_gen)
    # accumulate into an existing C with a padded pitch
    buf = torch.randn(M, N + 32, device=DEV, generator=g)
    c0 = buf[:, :N].clone()
    ops.gemm(A, B, False, tb, out=buf[:, :N], accumulate=True)
    close(buf[:, :N], (c0.double() + ref).float(), rtol=1e-5, atol=2e-5 * scale)


def test_tok_gemm_epilogues_batch_and_dropout_masks(ops):
    """bias / GELU (+ pre-activation aux) / ReLU / residual epilogues, the batched q-k-v form, and the SAME Philox
    dropout mask as the general kernel (element index row * N + col): zeros in the same places, survivors equal"""
    with ops.tok_gemm_min_rows(512):
        _tok_gemm_epilogue_checks(ops)


def _tok_gemm_epilogue_checks(ops):
    g = torch.Generator(device=DEV).manual_seed(11)
    M, N, K = 900, 512, 128
    A = torch.randn(M, K, device=DEV, generator=g)
    W = torch.randn(N, K, device=DEV, generator=g) * 0.2
    bias = torch.randn(N, device=DEV, generator=g)
    pre = (A.double() @ W.double().t() + bias.double()).float()
    aux = torch.empty((M, N), device=DEV)
    out = ops.gemm(A, W, False, True, bias=bias, epilogue=ops.EPI_BIAS_GELU, aux=aux)
    close(aux, pre, atol=2e-5)
    close(out, torch.nn.functional.gelu(pre), atol=2e-5)
    close(ops.gemm(A, W, False, True, bias=bias, epilogue=ops.EPI_BIAS_RELU), torch.relu(pre), atol=2e-5)
    close(ops.gemm(A, W, False, True, bias=bias, epilogue=ops.EPI_BIAS), pre, atol=2e-5)
    drop = (0.3, 1234, ops.dropout_ctr_hi(5, 2, ops.SITE_FF_ACT))
    d_new = ops.gemm(A, W, False, True, bias=bias, epilogue=ops.EPI_BIAS_GELU, aux=aux, drop=drop)
    with ops.precision("fp32"):
        d_gen = ops.gemm(A, W, False, True, bias=bias, epilogue=ops.EPI_BIAS_GELU, aux=aux, drop=drop)
    # zeros in the same places -- where the activation itself is not (nearly) zero: gelu(x) underflows to -0.0 around
    # x = -5.5 (1 + erf reaches 0), and the two kernels' pre-activations differ in the last bits there
    live = torch.nn.functional.gelu(pre).abs() > 1e-4
    assert torch.equal((d_new == 0) & live, (d_gen == 0) & live) and 0.25 < float((d_new == 0).float().mean()) < 0.35
    close(d_new, d_gen, atol=3e-5)
    res = torch.randn(M, N, device=DEV, generator=g)
    r_new = ops.gemm(A, W, False, True, bias=bias, epilogue=ops.EPI_BIAS_RESID, aux=res, drop=drop)
    with ops.precision("fp32"):
        r_gen = ops.gemm(A, W, False, True, bias=bias, epilogue=ops.EPI_BIAS_RESID, aux=res, drop=drop)
    close(r_new, r_gen, atol=3e-5)
    # batched: three adjacent [K, N] weights, one launch (the q / k / v projections of xlnet_layer.hip)
    T, D = 768, 128
    h = torch.randn(T, D, device=DEV, generator=g)
    w3 = torch.randn(3, D, D, device=DEV, generator=g) * 0.2
    qkv = torch.empty(3, T, D, device=DEV)
    ops.call("t4r_gemm_f32", ops._stream(), 0, 0, T, D, D, 1.0, h.data_ptr(), D, w3.data_ptr(), D, qkv.data_ptr(), D,
             None, 0, None, 0, 1, 0, 3, 0, D * D, T * D, 0.0, 0, 0)
    for z in range(3):
        close(qkv[z], (h.double() @ w3[z].double()).float(), atol=2e-5)
