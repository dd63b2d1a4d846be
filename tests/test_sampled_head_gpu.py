"""The sampled-softmax head (csrc/head.hip: t4r_sampled_logits_fwd / _bwd / _bwd_rows, t4r_log_uniform_sample) against the
oracle in float64.

Reference: O.sampled_logits on float64 copies of the inputs, autograd for the gradients.  Inputs at the project's weight scale
(x, W = 0.25 * randn), a vocabulary of 300 ids, the correction distribution of LogUniformSampler, sorted unique negatives >= 1,
and labels laid out so that every case (N > 1) has rows that label a drawn negative (accidental hits, a third of the rows),
rows that share a label (hit rows and others) and rows whose label is no negative.  Shapes: partial and whole 4-row workgroups,
row lengths that are not 16-byte loadable (D = 33), the row-wise | matrix-core switch at 3 | 4 negatives, the odd logits pitch
n_neg + 1 (64 at n_neg = 63), three temperatures.

Tolerance: the suite's standing rtol = atol = 2e-5 (tests/test_kernels_gpu.py: close).  The fp32 CPU evaluation of the same
oracle stays within 0.09 of it at N 130, D 256, S 100; a dropped term, row or correction is four orders of magnitude above it.
The comments next to the assertions give the largest error seen on the MI355X over all cases, as a fraction of the tolerance.

The device sampler is compared draw by draw with its restatement oracle/device_rng.py: log_uniform_draws."""
import functools

import numpy as np
import pytest
import torch

import device_rng as R
import t4r_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
V = 300
RTOL = ATOL = 2e-5
HIT32 = np.float32(-65504.0) / np.float32(100.0)        # finfo(fp16).min / 100 in fp32: the accidental-hit constant


@pytest.fixture(scope="module")
def ops():
    from transformers4rec_amd import ops as _ops

    return _ops


def cu(t):
    return t.to(DEV).contiguous()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def frac(a, ref):
    """largest |a - ref| as a fraction of the tolerance atol + rtol * |ref|"""
    a, ref = a.detach().cpu().double(), ref.detach().double()
    if a.numel() == 0:
        return 0.0
    return float(((a - ref).abs() / (ATOL + RTOL * ref.abs())).max())


def close(a, ref, what, case):
    f = frac(a, ref)
    print(f"sampled {what} {case}: {f:.4f} of the tolerance")
    torch.testing.assert_close(a.detach().cpu().double(), ref.detach().double(), rtol=RTOL, atol=ATOL, msg=lambda m: f"{what} {case}: {m}")


# N, D, S, T, h: the rows i with i % 3 == h label a negative.  N x D x S x T of the issue's cross product, trimmed: every value of
# every axis, every N with S on both sides of the 3 | 4 switch, every D with a partial workgroup and with several workgroups.
CASES = [
    (1, 8, 1, 1.0, 0), (1, 33, 4, 0.7, 1), (1, 256, 100, 2.0, 0),
    (3, 8, 3, 1.0, 1), (3, 64, 4, 0.7, 1), (3, 33, 63, 2.0, 0),
    (4, 33, 5, 1.0, 1), (4, 256, 64, 0.7, 2), (4, 8, 100, 2.0, 1), (4, 64, 1, 1.0, 1),
    (5, 8, 4, 2.0, 1), (5, 33, 3, 0.7, 1), (5, 64, 63, 1.0, 2), (5, 256, 5, 1.0, 0), (5, 33, 100, 0.7, 1),
    (130, 8, 63, 0.7, 1), (130, 33, 4, 1.0, 1), (130, 33, 64, 2.0, 0), (130, 64, 3, 2.0, 1), (130, 64, 100, 1.0, 2),
    (130, 256, 1, 0.7, 1), (130, 256, 5, 2.0, 1), (130, 256, 63, 1.0, 1), (130, 256, 100, 0.7, 1),
]


def _reference(x, y, W, neg, dist, T, dl):
    """fp64 oracle: logits, d x, d W (autograd) and the two halves of the row-sparse weight gradient (closed form)"""
    x64, W64 = x.double().requires_grad_(), W.double().requires_grad_()
    ref = O.sampled_logits(x64, y, W64, neg, dist.double(), T)
    ref.backward(dl.double())
    hits = y[:, None] == neg[None, :]
    g = dl.double() / T
    rows_pos = g[:, :1] * x.double()                                            # d W[y_row] from column 0, row by row
    rows_neg = torch.where(hits, torch.zeros_like(g[:, 1:]), g[:, 1:]).t() @ x.double()      # d W[neg_s], column by column
    return dict(logits=ref.detach(), dx=x64.grad, dW=W64.grad, hits=hits, rows_pos=rows_pos, rows_neg=rows_neg)


@functools.lru_cache(maxsize=None)
def _case(N, D, S, T, h):
    """inputs and their fp64 reference, computed once and shared (read-only) by the tests of one shape"""
    g = torch.Generator().manual_seed(N * 1000003 + D * 1009 + S * 7 + h)
    x, W = 0.25 * torch.randn(N, D, generator=g), 0.25 * torch.randn(V, D, generator=g)
    dist = O.unique_sampling_dist(O.log_uniform_dist(V, 1), 2 * S)
    perm = torch.randperm(V - 1, generator=g) + 1
    neg, pool = perm[:S].sort().values, perm[S:]
    y = torch.stack([neg[(i // 6) % S] if i % 3 == h else pool[(i // 3) % 4] for i in range(N)])
    dl = torch.randn(N, S + 1, generator=g)
    c = dict(x=x, W=W, dist=dist, neg=neg, y=y, dl=dl, T=T, **_reference(x, y, W, neg, dist, T, dl))
    hit_rows = c["hits"].any(1)
    assert int(neg.min()) >= 1 and bool((neg[1:] > neg[:-1]).all())
    if N > 1:                       # accidental hits, a label that is no negative, rows that share a label
        assert bool(hit_rows.any()) and not bool(hit_rows.all()) and y.unique().numel() < N
    if N == 130:
        assert 40 <= int(hit_rows.sum()) <= 46 and y[hit_rows].unique().numel() < int(hit_rows.sum())
    return c


def _fwd_rowwise(ops, c):
    """t4r_sampled_logits_fwd with a null workspace: the row-wise kernel whatever n_neg is"""
    from transformers4rec_amd._lib import call

    N, D = c["x"].shape
    S = c["neg"].numel()
    x, y, W, neg, dist = cu(c["x"]), cu(c["y"]), cu(c["W"]), cu(c["neg"]), cu(c["dist"])
    out = torch.full((N, S + 1), float("nan"), device=DEV)
    call("t4r_sampled_logits_fwd", torch.cuda.current_stream().cuda_stream, x.data_ptr(), y.data_ptr(), W.data_ptr(),
         neg.data_ptr(), dist.data_ptr(), out.data_ptr(), N, D, S, float(c["T"]), None)
    return out


@pytest.mark.parametrize("N,D,S,T,h", CASES)
def test_forward_both_forms(ops, N, D, S, T, h):
    c = _case(N, D, S, T, h)
    tag = (N, D, S, T)
    mc = ops.sampled_logits_fwd(cu(c["x"]), cu(c["y"]), cu(c["W"]), cu(c["neg"]), cu(c["dist"]), T).cpu()    # matrix cores for S >= 4
    rw = _fwd_rowwise(ops, c).cpu()
    hits = torch.cat([torch.zeros(N, 1, dtype=torch.bool), c["hits"]], 1)
    want = torch.tensor(HIT32 * (np.float32(1.0) / np.float32(T)))
    for name, out in (("matrix-core", mc), ("row-wise", rw)):
        assert out.shape == (N, S + 1)
        assert torch.equal(bits(out[hits]), bits(want).expand(int(hits.sum()))), name      # the constant, bit for bit
        close(out[~hits], c["logits"][~hits], f"fwd {name}", tag)      # MI355X: 0.16 of the tolerance (matrix cores), 0.03 (row-wise)
    close(mc, rw.double(), "fwd matrix-core vs row-wise", tag)         # MI355X: 0.15
    assert torch.equal(bits(mc[hits]), bits(rw[hits]))


@pytest.mark.parametrize("N,D,S,T,h", CASES)
def test_backward_dense(ops, N, D, S, T, h):
    c = _case(N, D, S, T, h)
    tag = (N, D, S, T)
    dW0 = 0.25 * torch.randn(V, D, generator=torch.Generator().manual_seed(5))        # d W is ACCUMULATED into
    dW, dl = cu(dW0), cu(c["dl"])
    dx = ops.sampled_logits_bwd(dl, cu(c["x"]), cu(c["y"]), cu(c["W"]), cu(c["neg"]), dW, T)
    close(dx, c["dx"], "bwd dx", tag)                                                 # MI355X: 0.09
    close(dW.cpu().double() - dW0.double(), c["dW"], "bwd dW", tag)                   # MI355X: 0.11
    untouched = torch.ones(V, dtype=torch.bool)
    untouched[c["y"]] = False
    untouched[c["neg"]] = False
    assert torch.equal(bits(dW.cpu()[untouched]), bits(dW0[untouched]))               # rows of no label and no negative
    want = c["dl"].clone()                                    # d logits comes back with exactly the hit entries zeroed
    want[:, 1:][c["hits"]] = 0.0
    assert torch.equal(bits(dl), bits(want))


@pytest.mark.parametrize("N,D,S,T,h", CASES)
def test_backward_rows(ops, N, D, S, T, h):
    c = _case(N, D, S, T, h)
    tag = (N, D, S, T)
    args = [cu(c[k]) for k in ("x", "y", "W", "neg")]
    dl = cu(c["dl"])
    dx, ids, rows = ops.sampled_logits_bwd_rows(dl, *args, T)
    assert torch.equal(ids.cpu(), torch.cat([c["y"], c["neg"]])) and rows.shape == (N + S, D)
    close(dx, c["dx"], "rows dx", tag)                                                # MI355X: 0.09
    close(rows[:N], c["rows_pos"], "rows[:N]", tag)                                   # MI355X: 0.004
    close(rows[N:], c["rows_neg"], "rows[N:]", tag)                                   # MI355X: 0.11
    want = c["dl"].clone()
    want[:, 1:][c["hits"]] = 0.0
    assert torch.equal(bits(dl), bits(want))
    table = torch.zeros(V, D, device=DEV)
    ops.scatter_rows_sorted(table, ids, rows)
    close(table, c["dW"], "rows scattered", tag)                                      # MI355X: 0.11
    dense = torch.zeros(V, D, device=DEV)
    dx_d = ops.sampled_logits_bwd(cu(c["dl"]), *args, dense, T)
    close(table, dense.cpu().double(), "rows vs dense dW", tag)                       # MI355X: 0.05
    assert torch.equal(bits(dx), bits(dx_d))                                          # d x: the same launches in both forms
    # a second run: the same bits (no atomics on this path at these sizes)
    dx2, ids2, rows2 = ops.sampled_logits_bwd_rows(cu(c["dl"]), *args, T)
    table2 = torch.zeros(V, D, device=DEV)
    ops.scatter_rows_sorted(table2, ids2, rows2)
    assert torch.equal(bits(dx2), bits(dx)) and torch.equal(bits(rows2), bits(rows)) and torch.equal(bits(table2), bits(table))


@pytest.mark.parametrize("N,D,S,T", [(5, 33, 6, 0.7), (130, 64, 100, 1.0)])
def test_backward_rows_duplicate_negatives(ops, N, D, S, T):
    """the row-sparse form has no distinctness precondition (only the dense form's header states one): negatives that repeat
    give one gradient row each and the sorted scatter sums them, as the oracle's indexing does by construction"""
    g = torch.Generator().manual_seed(N + S)
    x, W = 0.25 * torch.randn(N, D, generator=g), 0.25 * torch.randn(V, D, generator=g)
    dist = O.unique_sampling_dist(O.log_uniform_dist(V, 1), 2 * S)
    perm = torch.randperm(V - 1, generator=g) + 1
    neg = perm[:S // 2].repeat_interleave(2)[:S].sort().values                 # every negative twice
    y = torch.stack([neg[(2 * i) % S] if i % 3 == 1 else perm[S + i % 4] for i in range(N)])
    dl = torch.randn(N, S + 1, generator=g)
    assert neg.unique().numel() == S // 2
    ref = _reference(x, y, W, neg, dist, T, dl)
    assert int(ref["hits"].sum()) == 2 * int((torch.arange(N) % 3 == 1).sum())  # a hit row hits both copies
    tag = ("dup", N, D, S, T)
    dl_d = cu(dl)
    dx, ids, rows = ops.sampled_logits_bwd_rows(dl_d, cu(x), cu(y), cu(W), cu(neg), T)
    close(dx, ref["dx"], "rows dx", tag)                                              # MI355X: 0.07, 0.001, 0.07, 0.15 for the four comparisons
    close(rows[:N], ref["rows_pos"], "rows[:N]", tag)
    close(rows[N:], ref["rows_neg"], "rows[N:]", tag)
    table = torch.zeros(V, D, device=DEV)
    ops.scatter_rows_sorted(table, ids, rows)
    close(table, ref["dW"], "rows scattered", tag)
    want = dl.clone()
    want[:, 1:][ref["hits"]] = 0.0
    assert torch.equal(bits(dl_d), bits(want))


# ------------------------------------------------------------------------------------------ the sampler
BAND = 1e-12        # draws whose R^u lies this close (relative) to an integer may round the other way on the device


@pytest.mark.parametrize("min_id", [0, 1, 5])
@pytest.mark.parametrize("n,Rg", [(4099, 100_001), (4099, 2), (4099, 1_000_001), (300, 17), (4099, 3)])
def test_log_uniform_sample_equals_its_restatement(ops, n, Rg, min_id):
    """t4r_log_uniform_sample == device_rng.log_uniform_draws, draw by draw.  exp and log in double are the one place where
    the two may round differently: a draw whose R^u lies within 1e-12 (relative) of an integer may differ by one -- with
    these seeds no draw does (the closest comes to ~1e-10), which is asserted, so equality is demanded of every draw."""
    max_id = min_id + Rg - 1
    seed, ctr = 0x5EED0000 + Rg, R.dropout_ctr_hi(3, 0xFC, 0) + min_id
    pw = R.log_uniform_pow(seed, ctr, n, min_id, max_id)
    near = np.abs(pw - np.rint(pw)) <= BAND * pw
    assert int(near.sum()) == 0
    want = torch.from_numpy(R.log_uniform_draws(seed, ctr, n, min_id, max_id))
    got = ops.log_uniform_sample(n, min_id, max_id, seed, ctr, DEV).cpu()
    assert got.dtype == torch.int64 and int(got.min()) >= min_id and int(got.max()) < max_id
    diff = got != want
    assert not bool(diff.any()), (int(diff.sum()), got[diff][:5], want[diff][:5])
    if Rg == 2:
        assert bool((got == min_id).all())


def test_sampler_module_advances_its_stream(ops):
    """LogUniformSampler.sample: call k draws at stream position dropout_ctr_hi(k, 0xFC, 0) -- the restated draws, unique,
    sorted, truncated to max_n_samples -- so that consecutive steps train against different negatives"""
    import transformers4rec_amd as tr

    Vs, min_id, seed = 100_001, 1, 0x1234_5678_9ABC
    s = tr.LogUniformSampler(max_n_samples=100, max_id=Vs, min_id=min_id).to(DEV)
    s.seed = seed
    labels = torch.ones(3, dtype=torch.long, device=DEV)
    got = [s.sample(labels).cpu() for _ in range(3)]
    for k, neg in enumerate(got, 1):
        ctr = R.dropout_ctr_hi(k, 0xFC, 0)
        pw = R.log_uniform_pow(seed, ctr, s.n_sample, min_id, Vs)
        assert s.n_sample == 200 and int((np.abs(pw - np.rint(pw)) <= BAND * pw).sum()) == 0
        want = torch.from_numpy(np.unique(R.log_uniform_draws(seed, ctr, s.n_sample, min_id, Vs))[:100])
        assert torch.equal(neg, want), k
    assert not (torch.equal(got[0], got[1]) and torch.equal(got[1], got[2]))
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[1], got[2])
