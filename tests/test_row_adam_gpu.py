"""The row-sparse (lazy) Adam step (csrc/row_adam.hip: t4r_row_adam_step) on the GPU.

Held to the DENSE sequence the project runs without it, bit for bit on the rows that have a gradient: a zeroed [V, D] gradient,
ops.scatter_rows_sorted of the same (ids, rows), ops.adamw_step_ with the same hyper-parameters -- the segmented sum is the same
device code with the same geometry (csrc/seg_sum_kernel.h) and the update is adamw_element (csrc/adam_kernel.h).  Every other row of
param and of the two moments, and the guard floats around the three buffers, must keep their bits: the lazy step does not touch
them.  Twenty lazy steps are held to the float64 restatement (tests/row_adam_restatement.py) with the bound of
tests/test_adam_gpu.py, and one training step of two whole models to FusedAdam over both buckets."""
import numpy as np
import pytest
import torch

import row_adam_restatement as ra

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.25                      # guard value: exactly representable, never produced by a step
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)


@pytest.fixture(scope="module")
def ops():
    from transformers4rec_amd import ops as _ops

    return _ops


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def f32(x):
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ inputs
def make_ids(pattern, V, n, g):
    """-> (ids int64 [n], padding_idx)"""
    if n == 0:
        return torch.zeros(0, dtype=torch.int64), -1
    if pattern == "distinct":
        assert n <= V
        return torch.randperm(V, generator=g)[:n], -1
    if pattern == "zipf":               # P(rank k) ~ 1 / k over a random relabelling of the rows
        w = 1.0 / torch.arange(1, V + 1, dtype=torch.float64)
        relabel = torch.randperm(V, generator=g)
        return relabel[torch.multinomial(w, n, replacement=True, generator=g)], -1
    if pattern == "equal":              # every lookup hits one popular item: ONE run of n
        return torch.full((n,), min(3, V - 1), dtype=torch.int64), -1
    if pattern == "straddle":
        # sorted runs of lengths around the wave's chunk (16 positions), the workgroup (4 waves = 64 positions) and several
        # workgroups, starting at odd offsets: cut at one border, at many, and not at all
        lens, out, r = [5, 15, 17, 1, 63, 65, 33, 130, 2, 16, 64, 31, 257, 7], [], 0
        rows = torch.randperm(V, generator=g)
        while len(out) < n:
            ln = lens[r % len(lens)]
            out += [int(rows[r % V])] * ln
            r += 1
        ids = torch.tensor(out[:n], dtype=torch.int64)
        return ids[torch.randperm(n, generator=g)], -1
    if pattern == "ends":               # the first and the last row of the table, padding_idx = -1: id 0 counts
        ids = torch.randint(0, V, (n,), generator=g)
        ids[0], ids[n // 2], ids[-1] = 0, V - 1, 0
        ids[1] = V - 1
        return ids, -1
    if pattern == "padmix":             # padding ids (0), ids >= V and negative ids mixed in: all carry nothing
        ids = torch.randint(1, V, (n,), generator=g)
        junk = torch.tensor([0, V, V + 5, -3, 0, 2 * V + 1], dtype=torch.int64)
        where = torch.randperm(n, generator=g)[: max(1, n // 3)]
        ids[where] = junk[torch.arange(where.numel()) % junk.numel()]
        return ids, 0
    raise KeyError(pattern)


def touched_rows(ids, V, pad):
    keep = (ids != pad) & (ids >= 0) & (ids < V)
    return torch.unique(ids[keep])


class Arena:
    """param, exp_avg, exp_avg_sq [V, D] as slices of larger SENT-filled buffers.  guard % 4 == 0 keeps the slices 16-byte
    aligned (the float4 path where D % 4 == 0); guard % 4 != 0 takes the scalar path at any D."""

    def __init__(self, V, D, g, guard=64):
        self.V, self.D, self.guard = V, D, guard
        self.init = [0.1 * torch.randn(V, D, generator=g), 0.05 * torch.randn(V, D, generator=g),
                     1e-3 * torch.rand(V, D, generator=g) + 1e-7]                     # p, m, v > 0
        self.reset()

    def reset(self):
        self.bufs = []
        for t in self.init:
            b = torch.full((self.guard + t.numel() + self.guard,), SENT, device=DEV)
            b[self.guard: self.guard + t.numel()] = t.reshape(-1).to(DEV)
            self.bufs.append(b)
        self.pmv = [b[self.guard: self.guard + self.V * self.D].view(self.V, self.D) for b in self.bufs]

    def guards_intact(self):
        return all(bool((b[: self.guard] == SENT).all()) and bool((b[self.guard + self.V * self.D:] == SENT).all()) for b in self.bufs)


def dense_sequence(ops, init, ids, rows, pad, step, hp, decoupled, gs):
    """what the project does without the lazy step, on copies: zeroed gradient, sorted scatter, fused AdamW over every element"""
    p, m, v = [t.to(DEV).clone() for t in init]
    grad = torch.zeros_like(p)
    if ids.numel():
        ops.scatter_rows_sorted(grad, ids.to(DEV), rows.to(DEV).contiguous(), pad)
    ops.adamw_step_(p.view(-1), grad.view(-1), m.view(-1), v.view(-1), step, decoupled=decoupled, grad_scale=gs, zero_grad=False, **hp)
    return p, m, v


def check_one_step(ops, V, D, n, pattern, step, hp=HP, decoupled=False, gs=1.0, guard=64, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * V + 13 * D + n + step)
    ids, pad = make_ids(pattern, V, n, g)
    rows = torch.randn(n, D, generator=g) * 10.0 ** (4.0 * torch.rand(n, 1, generator=g) - 3.0)
    ar = Arena(V, D, g, guard)
    want = dense_sequence(ops, ar.init, ids, rows, pad, step, hp, decoupled, gs)
    t = touched_rows(ids, V, pad)
    still = torch.ones(V, dtype=torch.bool)
    still[t] = False
    got = []
    for _ in range(2):                                                   # the second run: the same bits
        ar.reset()
        ops.row_adam_step_(*ar.pmv, ids.to(DEV), rows.to(DEV), step, decoupled=decoupled, grad_scale=gs, padding_idx=pad, **hp)
        torch.cuda.synchronize()
        assert ar.guards_intact(), (V, D, n, pattern)
        got.append([x.cpu().clone() for x in ar.pmv])
    for k, name in enumerate(("param", "exp_avg", "exp_avg_sq")):
        assert same_bits(got[0][k][t], want[k].cpu()[t]), (name, V, D, n, pattern, step)           # touched rows: the dense bits
        assert same_bits(got[0][k][still], ar.init[k][still]), (name, V, D, n, pattern, step)      # every other row: untouched
        assert same_bits(got[0][k], got[1][k]), (name, V, D, n, pattern, step)
    if n and pattern != "padmix":
        assert t.numel() > 0 and not same_bits(got[0][0][t], ar.init[0][t])                        # the step did move them
    return t


# ------------------------------------------------------------------------------------------------ 1. one step, dense bits
@pytest.mark.parametrize("V,D,n,pattern,step", [
    (7, 1, 257, "zipf", 1),
    (7, 4, 1, "distinct", 2),
    (7, 6, 5000, "equal", 1000),            # one run of 5000 in a 7-row table
    (7, 64, 5000, "equal", 1),
    (7, 130, 257, "ends", 2),
    (1000, 1, 5000, "zipf", 2),
    (1000, 4, 257, "ends", 1),
    (1000, 6, 5000, "padmix", 1000),
    (1000, 64, 0, "distinct", 1),           # n = 0: nothing launches, nothing moves
    (1000, 64, 1, "distinct", 1000),
    (1000, 64, 257, "distinct", 2),
    (1000, 64, 5000, "zipf", 1),
    (1000, 64, 5000, "straddle", 2),
    (1000, 64, 5000, "padmix", 1),
    (1000, 130, 5000, "straddle", 1000),
    (1000, 130, 5000, "zipf", 2),
    (1000, 130, 1, "distinct", 1),
])
def test_one_step_matches_the_dense_sequence_bit_for_bit(ops, V, D, n, pattern, step):
    t = check_one_step(ops, V, D, n, pattern, step)
    if pattern == "ends":
        assert 0 in t.tolist() and V - 1 in t.tolist()
    if pattern == "padmix":
        assert 0 not in t.tolist() and int(t.max()) < V
    if pattern == "equal":
        assert t.tolist() == [min(3, V - 1)]


@pytest.mark.parametrize("D", [4, 64])
def test_unaligned_buffers_take_the_scalar_path(ops, D):
    """the three buffers 4 bytes past a 16-byte boundary: D % 4 == 0 alone does not allow 16-byte accesses"""
    check_one_step(ops, 1000, D, 5000, "zipf", 2, guard=65)


# ------------------------------------------------------------------------------------------------ 2. weight decay, grad_scale
@pytest.mark.parametrize("D", [6, 64])
@pytest.mark.parametrize("decoupled", [False, True])
def test_weight_decay_forms_and_grad_scale(ops, D, decoupled):
    hp = dict(HP, weight_decay=0.01, lr=1e-2)
    check_one_step(ops, 1000, D, 5000, "zipf", 2, hp=hp, decoupled=decoupled, gs=0.125, seed=1)
    check_one_step(ops, 7, D, 257, "zipf", 1000, hp=hp, decoupled=decoupled, gs=0.125, seed=2)


# ------------------------------------------------------------------------------------------------ 3. row pitch, two entries
@pytest.mark.parametrize("D,ld", [(64, 72), (64, 67), (6, 9), (130, 132)])
def test_row_pitched_gradient_rows(ops, D, ld):
    V, n = 1000, 5000
    g = torch.Generator().manual_seed(D + ld)
    ids, pad = make_ids("zipf", V, n, g)
    wide = torch.randn(n, ld, generator=g).to(DEV)
    rows = wide[:, :D]
    assert rows.stride(0) == ld and not rows.is_contiguous()
    ar = Arena(V, D, g)
    ops.row_adam_step_(*ar.pmv, ids.to(DEV), rows, 3, padding_idx=pad, **HP)
    pitched = [x.cpu().clone() for x in ar.pmv]
    ar.reset()
    ops.row_adam_step_(*ar.pmv, ids.to(DEV), rows.contiguous(), 3, padding_idx=pad, **HP)
    for a, b in zip(pitched, ar.pmv):
        assert same_bits(a, b)
    assert ar.guards_intact()
    want = dense_sequence(ops, ar.init, ids, rows.cpu(), pad, 3, HP, False, 1.0)
    t = touched_rows(ids, V, pad)
    for a, b in zip(pitched, want):
        assert same_bits(a[t], b.cpu()[t])


def test_two_pending_entries_equal_one_concatenated_entry(ops):
    """RowSparseAdam.step sums a table's entries as ONE list in arrival order; entries with different padding ids (the lookups'
    0, a sampled head's -1) keep each its own"""
    from transformers4rec_amd import optim

    V, D = 300, 20
    g = torch.Generator().manual_seed(5)
    p0 = 0.1 * torch.randn(V, D, generator=g)
    a = torch.nn.Parameter(p0.clone().to(DEV))
    b = torch.nn.Parameter(p0.clone().to(DEV))
    two, one = optim.RowSparseAdam([a], weight_decay=0.01), optim.RowSparseAdam([b], weight_decay=0.01)
    for _ in range(2):
        ids1, _ = make_ids("zipf", V, 400, g)
        ids1[::5] = 0                                           # the lookups' padding id ...
        ids2, _ = make_ids("zipf", V, 150, g)
        ids2[::7] = 0                                           # ... is an item like any other for the head
        rows1, rows2 = torch.randn(400, D, generator=g).to(DEV), torch.randn(150, D, generator=g).to(DEV)
        two.add_rows(a, ids1.to(DEV), rows1, padding_idx=0)
        two.add_rows(a, ids2.to(DEV), rows2, padding_idx=-1)
        cat = torch.cat([torch.where(ids1 == 0, torch.full_like(ids1, V), ids1), ids2])
        one.add_rows(b, cat.to(DEV), torch.cat([rows1, rows2]), padding_idx=-1)
        two.step()
        one.step()
        assert two._pending == [] and one._pending == []
    assert two.step_count == one.step_count == 2
    assert same_bits(a, b) and same_bits(two.state[0][0], one.state[0][0]) and same_bits(two.state[0][1], one.state[0][1])
    assert not same_bits(a[0], p0[0])                            # row 0 got the head's gradient


# ------------------------------------------------------------------------------------------------ 4. twenty steps against fp64
def units(p, p_ref, lr):
    """max over the elements of |p - p_ref| in units of 2^-24 * (|p_ref| + lr): as tests/test_adam_gpu.py"""
    p_ref = np.asarray(p_ref, dtype=np.float64)
    return float((np.abs(np.asarray(p, dtype=np.float64) - p_ref) / (2.0 ** -24 * (np.abs(p_ref) + lr))).max())


def test_twenty_lazy_steps_against_fp64(ops):
    """V 300, D 20, a different Zipf subset of 400 lookups each step, gradient magnitudes spread over 1e-4 .. 1e2 as in
    tests/test_adam_gpu.py, hyper-parameters rounded to fp32 first.  The bound is that file's, after every step:
        E_dev <= 2 * E_f32 + 4        in units of 2^-24 * (|p_ref| + lr)
    with E_f32 the error of the restatement run in float32 on the same inputs (the part torch's fp32 CPU Adam plays there).
    Rows a step does not name keep their bits in that step (the lazy rule)."""
    V, D, n, steps = 300, 20, 400, 20
    hp = dict(lr=f32(1e-2), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8), weight_decay=f32(0.0))
    g = torch.Generator().manual_seed(20)
    p0 = 1e-3 * torch.randn(V, D, generator=g)
    dev = [p0.to(DEV).clone(), torch.zeros(V, D, device=DEV), torch.zeros(V, D, device=DEV)]
    r64 = [p0.double().numpy().copy(), np.zeros((V, D)), np.zeros((V, D))]
    r32 = [p0.numpy().copy(), np.zeros((V, D), np.float32), np.zeros((V, D), np.float32)]
    worst = 0.0
    for step in range(1, steps + 1):
        ids, pad = make_ids("zipf", V, n, g)
        rows = torch.randn(n, D, generator=g) * 10.0 ** (6.0 * torch.rand(n, D, generator=g) - 4.0)
        before = [x.cpu().clone() for x in dev]
        ops.row_adam_step_(*dev, ids.to(DEV), rows.to(DEV), step, padding_idx=pad, **hp)
        kw = dict(lr=hp["lr"], betas=hp["betas"], eps=hp["eps"])
        t64 = ra.lazy_adam_step(*r64, ids.numpy(), rows.numpy(), step, **kw)
        ra.lazy_adam_step(*r32, ids.numpy(), rows.numpy(), step, **kw)
        t = touched_rows(ids, V, pad)
        assert t.tolist() == t64.tolist() and 0 < t.numel() < V
        still = torch.ones(V, dtype=torch.bool)
        still[t] = False
        for a, b in zip(dev, before):
            assert same_bits(a.cpu()[still], b[still]), step
        e_dev, e_f32 = units(dev[0].cpu().numpy(), r64[0], hp["lr"]), units(r32[0], r64[0], hp["lr"])
        print(f"row adam step={step}: E_dev={e_dev:.2f} E_f32={e_f32:.2f} touched={t.numel()}")
        worst = max(worst, e_dev - (2.0 * e_f32 + 4.0))
        assert e_dev <= 2.0 * e_f32 + 4.0, (step, e_dev, e_f32)
    print(f"row adam: largest E_dev - (2 E_f32 + 4) over {steps} steps: {worst:.2f}")


# ------------------------------------------------------------------------------------------------ 5. whole models
def _build(arch, masking, weight_tying):
    import transformers4rec_amd as tr

    V, L, d = 500, 8, 32
    torch.manual_seed(0)
    schema = tr.session_schema(V - 1, L)
    inputs = tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=L, masking=masking, aggregation="concat",
                                                    embedding_dim_default=d)
    kw = dict(d_model=d, n_head=2, n_layer=2, total_seq_length=L, dropout=0.0)
    cfg = (tr.GPT2Config if arch == "gpt2" else tr.XLNetConfig).build(**kw)
    model = cfg.to_torch_model(inputs, tr.NextItemPredictionTask(weight_tying=weight_tying, sampled_softmax=True, max_n_samples=50))
    batch = tr.random_data_from_schema(schema, 16, L, min_session_length=3, seed=4)["item_id"]
    return model.to(DEV), batch.to(DEV)


def _train_step(model, batch, opts):
    out = model({"item_id": batch}, training=True)
    out["loss"].backward()
    for o in opts:
        o.step()
    torch.cuda.synchronize()
    return float(out["loss"].detach())


def _sparse_pair(model):
    """the recipe of optim.RowSparseAdam's docstring -> (tables by name, FusedAdam over the rest, the attached lazy optimizer)"""
    from transformers4rec_amd import optim

    sparse = dict(optim.row_sparse_tables(model))
    dense = optim.FlatParams((n, p) for n, p in model.named_parameters() if n not in sparse)
    return sparse, optim.FusedAdam([dense], lr=LR), optim.RowSparseAdam(sparse.values(), lr=LR).attach()


MODELS = [("gpt2", "clm", True), ("xlnet", "mlm", False)]
LR = 1e-3
# Parameters whose gradient the library sums through fp32 atomics, in arrival order: t4r_add_pos_bwd, the GPT-2 / BERT position
# embedding (csrc/elementwise.hip: add_pos_bwd_kernel; tests/test_abi_redzone_gpu.py: ATOMIC_ENTRIES holds that entry to a value
# tolerance, not to bits).  Two runs of FusedAdam over both buckets differ from each other there (measured: 12 - 16 of 256
# elements by 1 ulp), so no optimizer can be held to its bits.  What does hold for any order of the sum: a first Adam step
# from zero moments moves an element by lr * |g| / (|g| + eps) < lr, so two first steps from one start differ by less than 2 lr.
ATOMIC_GRADIENT = ("transformer.wpe.weight",)
FIRST_STEP_SPAN = 2.0 * LR * (1.0 + 2.0 ** -10)          # 2 lr and room for the handful of fp32 roundings of the update


def _first_steps(arch, masking, weight_tying, record=None):
    """one training step of two equal models from fresh optimizers, weight_decay 0: FusedAdam over both buckets (a) and
    FusedAdam(dense) + RowSparseAdam(tables) (b) -> (a's parameters, b's parameters, b's tables); record: a list that receives
    b's (table, valid ids) entries in arrival order"""
    from transformers4rec_amd import optim

    model_a, batch = _build(arch, masking, weight_tying)
    model_b, _ = _build(arch, masking, weight_tying)
    for (_, pa), (_, pb) in zip(model_a.named_parameters(), model_b.named_parameters()):
        assert same_bits(pa, pb)
    dense_a, tables_a = optim.flatten_model(model_a)
    loss_a = _train_step(model_a, batch, [optim.FusedAdam([dense_a, tables_a], lr=LR)])
    sparse, opt_d, opt_s = _sparse_pair(model_b)
    if record is not None:
        collect = opt_s.add_rows

        def recording_add_rows(tab, ids, rows, padding_idx=-1):
            ids = ids.reshape(-1)
            record.append((tab, ids[(ids != padding_idx) & (ids >= 0) & (ids < tab.shape[0])].cpu()))
            collect(tab, ids, rows, padding_idx)

        opt_s.add_rows = recording_add_rows
    loss_b = _train_step(model_b, batch, [opt_d, opt_s])
    opt_s.detach()
    assert loss_a == loss_b and np.isfinite(loss_a)
    pa, pb = dict(model_a.named_parameters()), dict(model_b.named_parameters())
    assert list(pa) == list(pb)
    return pa, pb, sparse


def _hold_to_bits(arch, pa, pb, looser_rows=None):
    """every parameter of b bit-equal to a's; ATOMIC_GRADIENT parameters, and the rows looser_rows[name] of a table, are held
    to FIRST_STEP_SPAN instead (and must be finite); every figure is printed before anything is asserted"""
    looser_rows = looser_rows or {}
    differing = []
    for n, p in pa.items():
        a, b = p.detach().cpu(), pb[n].detach().cpu()
        d = bits(a) != bits(b)
        loose = torch.zeros_like(d)
        if n.endswith(ATOMIC_GRADIENT):
            loose[:] = True
        if n in looser_rows:
            loose[looser_rows[n]] = True
        if bool(d.any()):
            print(f"{arch}: {n}: {int(d.sum())} of {d.numel()} elements differ ({int((d & ~loose).sum())} of them held to bits), "
                  f"max |diff| {float((a - b).abs().max()):.3e}, rows {d.view(d.shape[0], -1).any(1).nonzero().view(-1).tolist()[:20]}")
        if bool((d & ~loose).any()) or not bool(torch.isfinite(b).all()) or float((a - b).abs().max()) > FIRST_STEP_SPAN:
            differing.append(n)
    assert not differing, differing


@pytest.mark.parametrize("arch,masking", [("gpt2", "clm"), ("xlnet", "mlm")])
def test_whole_model_first_step_equals_fused_adam(arch, masking):
    """One training step from fresh optimizers, weight_decay 0, of a model with an UNTIED sampled head (the library's default:
    NextItemPredictionTask(weight_tying=False)): FusedAdam over both buckets against FusedAdam(dense) + RowSparseAdam(tables).
    Each table receives one entry -- the item table the lookups' rows, output_layer the head's -- and with zero moments and a zero
    gradient the dense step leaves a row where it is, so every parameter must agree bit for bit (the position embedding of
    GPT-2, whose gradient the dense path itself does not reproduce from run to run: see ATOMIC_GRADIENT).
    Measured on the MI355X: see DESIGN.md section 4.8."""
    pa, pb, sparse = _first_steps(arch, masking, False)
    assert len(sparse) == 2
    _hold_to_bits(arch, pa, pb)


def test_tied_model_first_step_differs_only_where_two_entries_meet():
    """The GPT-2 CLM model with the TIED sampled head: the item table receives two entries in one step, the head's rows and the
    lookups'.  RowSparseAdam sums a table's entries as ONE list in arrival order, ((h1 + h2) + l1) + l2; FusedAdam's dense route
    adds two separately summed scatters, (h1 + h2) + (l1 + l2): for a row that BOTH entries name the two gradients can differ
    in their last bits (measured on the MI355X: 2 of 16 000 elements by 1 ulp, 9.3e-10, rows 264 and 270, each named twice by
    either entry; 56 rows are named by both).  Every row that at most one entry names, and every other parameter, is held to
    bits; the shared rows to FIRST_STEP_SPAN."""
    record = []
    pa, pb, sparse = _first_steps("gpt2", "clm", True, record)
    (name, table), = sparse.items()
    assert len(record) == 2 and all(t is table for t, _ in record)
    counts = [torch.bincount(ids, minlength=table.shape[0]) for _, ids in record]
    both = (counts[0] > 0) & (counts[1] > 0)
    assert 0 < int(both.sum()) < int(((counts[0] > 0) | (counts[1] > 0)).sum())
    _hold_to_bits("gpt2-tied", pa, pb, {name: both})


@pytest.mark.parametrize("arch,masking,weight_tying", MODELS)
def test_whole_model_lazy_steps_touch_named_rows_only(arch, masking, weight_tying):
    """Four training steps with the pair: finite losses; the table rows no lookup and no head row ever named keep their initial
    bits, the named ones move; no dense gradient is made for a table; a table maximum an earlier FusedAdam left is dropped."""
    model_b, batch = _build(arch, masking, weight_tying)
    sparse, opt_d, opt_s = _sparse_pair(model_b)
    init = {n: p.detach().cpu().clone() for n, p in sparse.items()}
    seen = {id(p): [] for p in sparse.values()}
    collect = opt_s.add_rows

    def recording_add_rows(tab, ids, rows, padding_idx=-1):
        ids = ids.reshape(-1)
        seen[id(tab)].append(ids[(ids != padding_idx) & (ids >= 0) & (ids < tab.shape[0])].cpu())
        collect(tab, ids, rows, padding_idx)

    opt_s.add_rows = recording_add_rows
    for p in sparse.values():
        p._t4r_w_amax = ("stale",)                              # what an earlier FusedAdam over this table would have left
    for k in range(4):
        assert np.isfinite(_train_step(model_b, torch.roll(batch, k, 0), [opt_d, opt_s]))
        for p in sparse.values():
            assert not hasattr(p, "_t4r_w_amax")
            assert p.grad is None                               # no dense gradient was ever made
    assert opt_s.step_count == 4 and opt_s._pending == []
    for n, p in sparse.items():
        named = torch.unique(torch.cat(seen[id(p)]))
        never = torch.ones(p.shape[0], dtype=torch.bool)
        never[named] = False
        assert 0 < int(never.sum()) < p.shape[0], n
        assert same_bits(p.detach().cpu()[never], init[n][never]), n
        assert not same_bits(p.detach().cpu()[named], init[n][named]), n
    opt_s.detach()
