"""Global-norm clipping across dense buckets and row-sparse tables on the GPU (csrc/row_adam.hip: t4r_row_adam_reduce,
t4r_row_adam_apply; include/t4r_hip_rowclip.h) and its driver optim.FusedAdam(max_grad_norm=).link(RowSparseAdam).

  * the norm partials: their sum against the float64 sum of squares of the DENSE sequence's gradient (a zeroed [V, D] buffer +
    ops.scatter_rows_sorted, whose fp32 values are the kernel's compact rows bit for bit), to rtol 1e-12.  Derived, not measured:
    the device squares and adds in double, a float squared is exact in double, and a double sum of at most 2^31 non-negative
    terms is good to n * 2^-53 relative whatever its order (tests/test_optim_clip_gpu.py uses the same bound).
  * the apply: the bits of the dense sequence (zeroed gradient, sorted scatter, ops.adamw_step_ with the SAME coefficient tensor) on
    the touched rows; every other row and the guard floats keep their bits; with no coefficient the bits of ops.row_adam_step_.
  * the linked pair: the joint norm to ONE fp32 ulp of float64 (only the final rounding can differ), and the same coefficient
    in the buckets' and the tables' steps.
  * twenty clipped lazy steps against the float64 restatement (tests/row_clip_restatement.py) under tests/test_adam_gpu.py's
    bound, one training step of two whole models against FusedAdam over both buckets, and red zones round every buffer."""
import math

import numpy as np
import pytest
import torch

import row_clip_restatement as rc
import test_abi_redzone_gpu as rz
from test_optim_clip_gpu import coef_of, ulps_apart
from test_row_adam_gpu import Arena, bits, f32, make_ids, same_bits, touched_rows, units

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = -7.0                     # fills the partial slots before a call: a sum of squares is never negative
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
WG = 256 * 4                      # elements one workgroup covers per trip (256 threads x float4)


@pytest.fixture(scope="module")
def ops():
    from transformers4rec_amd import ops as _ops

    return _ops


def spread_rows(n, D, g):
    """gradient rows with magnitudes spread over 1e-3 .. 1e1 per lookup (tests/test_row_adam_gpu.py's)"""
    return torch.randn(n, D, generator=g) * 10.0 ** (4.0 * torch.rand(n, 1, generator=g) - 3.0)


def dense_gradient(ops, V, D, ids, rows, pad):
    """the gradient the dense route would hold: zeroed [V, D] + the sorted scatter (device tensor)"""
    grad = torch.zeros(V, D, device=DEV)
    if ids.numel():
        ops.scatter_rows_sorted(grad, ids.to(DEV), rows.to(DEV).contiguous(), pad)
    return grad


def sumsq64(t):
    return float(t.double().square().sum())


def reduce_checked(ops, ids, rows, V, pad, extra=16):
    """ops.row_adam_reduce_ into a poisoned buffer -> (partials written [count] on the host, state); checks the count and that
    no slot beyond it was written"""
    n, D = ids.numel(), rows.shape[1]
    want = ops.row_grad_sumsq_parts(n, D)
    part = torch.full((want + extra,), POISON, device=DEV, dtype=torch.float64)
    cnt, st = ops.row_adam_reduce_(ids, rows, V, pad, part)
    pc = part.cpu()
    assert cnt == want == min(2048, max(1, (n * D // 4 + 255) // 256)) if n else cnt == want == 0
    assert bool((pc[cnt:] == POISON).all()), "a slot beyond the returned count was written"
    assert bool((pc[:cnt] >= 0).all()), "a slot below the returned count was left unwritten"
    return pc[:cnt].clone(), st


# ------------------------------------------------------------------------------------------------ 1. the norm partials
# (V, D, n, pattern, row pitch or None, seed): the smallest shapes that reach each path.  U = the number of distinct valid ids.
PART_CASES = [
    (7, 1, 0, "distinct", None, 0),           # n = 0: nothing launches, no slot is written
    (7, 1, 1, "distinct", None, 0),           # one float: all scalar tail
    (7, 3, 17, "zipf", None, 0),
    (7, 4, 1, "distinct", None, 0),           # one float4
    (7, 4, 5000, "equal", None, 0),           # one run of 5000 -> U = 1: 19 of the 20 workgroups lie wholly past U D
    (7, 130, 17, "zipf", None, 0),
    (7, 3, 5000, "zipf", 5, 0),               # pitched rows
    (1000, 1, 17, "distinct", None, 0),       # U D = 17: float4s and a scalar tail of 1
    (1000, 1, 5000, "zipf", None, 0),
    (1000, 3, 17, "padmix", None, 0),         # ids equal to padding, out of range and negative
    (1000, 3, 5000, "zipf", None, 0),         # U D crosses one workgroup's 1024 elements
    (1000, 4, 17, "distinct", None, 0),
    (1000, 4, 5000, "padmix", None, 0),
    (1000, 4, 5000, "zipf", 7, 0),            # pitched, the pitch no multiple of 4
    (1000, 130, 1, "distinct", None, 0),      # U D = 130: a scalar tail of 2
    (1000, 130, 17, "distinct", 132, 0),
    (1000, 130, 5000, "zipf", None, 0),
    (1000, 130, 5000, "equal", None, 0),      # U = 1 under a grid of 635 workgroups
]


def check_partials(ops, V, D, n, pattern, ld, seed, ids=None):
    g = torch.Generator().manual_seed(1000 * seed + 7 * V + 13 * D + n)
    pad = -1
    if ids is None:
        ids, pad = make_ids(pattern, V, n, g)
    rows = spread_rows(n, ld or D, g).to(DEV)[:, :D]
    assert ld is None or (rows.stride(0) == ld and (n < 2 or not rows.is_contiguous()))
    ids_d = ids.to(DEV)
    want = sumsq64(dense_gradient(ops, V, D, ids, rows, pad))
    U = int(touched_rows(ids, V, pad).numel())
    p1, _ = reduce_checked(ops, ids_d, rows, V, pad)
    p2, _ = reduce_checked(ops, ids_d, rows, V, pad)
    got = float(p1.sum())
    print(f"partials V={V} D={D} n={n} {pattern} ld={ld}: U={U} U*D={U * D} count={p1.numel()} sum={got!r} float64={want!r} "
          f"rel={abs(got - want) / want if want else 0.0:.2e}")
    assert abs(got - want) <= 1e-12 * want, (got, want)
    assert torch.equal(p1.view(torch.int64), p2.view(torch.int64)), "the partials differ between two runs"
    # the workgroups whose elements all lie past U * D stored an exact 0.0
    first_idle = (U * D + WG - 1) // WG
    assert bool((p1[first_idle:] == 0.0).all()) and (first_idle == 0 or float(p1[:first_idle].min()) > 0.0)
    return U, p1


@pytest.mark.parametrize("V,D,n,pattern,ld,seed", PART_CASES)
def test_partials_sum_to_the_dense_gradients_sum_of_squares(ops, V, D, n, pattern, ld, seed):
    U, part = check_partials(ops, V, D, n, pattern, ld, seed)
    if pattern == "equal":
        assert U == 1 and part.numel() > 1
    if (V, D, n, pattern) == (1000, 3, 5000, "zipf"):
        assert U * D > WG and part.numel() > (U * D + WG - 1) // WG          # more than one busy workgroup, and idle ones
    if (V, D, n) in ((1000, 1, 17), (1000, 130, 1)):
        assert (U * D) % 4 != 0 and U * D > 4                                # float4s and a scalar tail


def test_partials_of_lookups_that_are_all_padding(ops):
    """U = 0: every lookup is padding, out of range or negative -- every one of the count's slots is an exact 0.0"""
    V, D, n = 1000, 4, 5000
    ids = torch.tensor([0, V, V + 5, -3, 0, 2 * V + 1], dtype=torch.int64).repeat(n // 6 + 1)[:n]
    rows = spread_rows(n, D, torch.Generator().manual_seed(3)).to(DEV)
    part, _ = reduce_checked(ops, ids.to(DEV), rows, V, 0)
    assert part.numel() == 20 and bool((part == 0.0).all())


def test_partials_at_the_capped_grid(ops):
    """n 65 536 near-distinct ids, V 100 000, D 128 (a 32 MB compact buffer): the smallest size at which the count is at its
    cap of 2048 AND a thread's grid-stride loop takes its four-loads-in-flight form (3 trips of 2048 x 1024 elements + 4 <= U D)"""
    V, D, n = 100_000, 128, 65_536
    g = torch.Generator().manual_seed(11)
    ids = torch.randperm(V, generator=g)[:n]
    ids[::97] = ids[1::97][: ids[::97].numel()]                 # 676 lookups repeat their neighbour's id
    U, part = check_partials(ops, V, D, n, "near-distinct", None, 0, ids=ids)
    assert part.numel() == 2048 and U * D >= 3 * 2048 * WG + 4 and U < n


# ------------------------------------------------------------------------------------------------ 2. the apply: dense bits
def dense_sequence(ops, init, ids, rows, pad, step, hp, decoupled, gs, coef):
    """what the project does without the lazy step, on copies: zeroed gradient, sorted scatter, fused AdamW over every element
    with the coefficient tensor `coef` (or None)"""
    p, m, v = [t.to(DEV).clone() for t in init]
    grad = dense_gradient(ops, p.shape[0], p.shape[1], ids, rows, pad)
    ops.adamw_step_(p.view(-1), grad.view(-1), m.view(-1), v.view(-1), step, decoupled=decoupled, grad_scale=gs, zero_grad=False,
                    clip_coef=coef, **hp)
    return p, m, v


def check_apply(ops, V, D, n, pattern, step, hp=HP, decoupled=False, gs=1.0, guard=64, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * V + 13 * D + n + step)
    ids, pad = make_ids(pattern, V, n, g)
    rows = spread_rows(n, D, g)
    ar = Arena(V, D, g, guard)
    ids_d, rows_d = ids.to(DEV), rows.to(DEV)
    t = touched_rows(ids, V, pad)
    still = torch.ones(V, dtype=torch.bool)
    still[t] = False
    for c in (0.37, 1.0, None):
        coef = None if c is None else torch.tensor([c], device=DEV)
        want = dense_sequence(ops, ar.init, ids, rows, pad, step, hp, decoupled, gs, coef)
        got = []
        for _ in range(2):                                                   # the second run: the same bits
            ar.reset()
            _, st = reduce_checked(ops, ids_d, rows_d, V, pad)
            ops.row_adam_apply_(*ar.pmv, st, step, decoupled=decoupled, grad_scale=gs, clip_coef=coef, **hp)
            torch.cuda.synchronize()
            assert ar.guards_intact(), (V, D, n, pattern, c)
            got.append([x.cpu().clone() for x in ar.pmv])
        for k, name in enumerate(("param", "exp_avg", "exp_avg_sq")):
            assert same_bits(got[0][k][t], want[k].cpu()[t]), (name, V, D, n, pattern, step, c)         # touched rows: the dense bits
            assert same_bits(got[0][k][still], ar.init[k][still]), (name, V, D, n, pattern, step, c)    # every other row: untouched
            assert same_bits(got[0][k], got[1][k]), (name, V, D, n, pattern, step, c)
        if c != 0.37:                                                        # no coefficient, or 1.0: the unclipped lazy step's bits
            ar.reset()
            ops.row_adam_step_(*ar.pmv, ids_d, rows_d, step, decoupled=decoupled, grad_scale=gs, padding_idx=pad, **hp)
            for k in range(3):
                assert same_bits(got[0][k], ar.pmv[k]), (k, V, D, n, pattern, step, c)
        elif n and t.numel():
            plain = dense_sequence(ops, ar.init, ids, rows, pad, step, hp, decoupled, gs, None)
            assert not same_bits(got[0][1][t], plain[1].cpu()[t])           # 0.37 did reach the first moment
    return t


@pytest.mark.parametrize("V,D,n,pattern,step", [
    (7, 1, 17, "zipf", 1),
    (7, 3, 5000, "equal", 1000),
    (7, 4, 1, "distinct", 2),
    (7, 130, 17, "ends", 2),
    (1000, 1, 5000, "zipf", 2),
    (1000, 3, 5000, "padmix", 1000),
    (1000, 4, 0, "distinct", 1),             # n = 0: nothing launches, nothing moves
    (1000, 4, 5000, "zipf", 1),
    (1000, 130, 1, "distinct", 1),
    (1000, 130, 5000, "zipf", 2),
])
def test_apply_matches_the_dense_step_with_the_same_coefficient(ops, V, D, n, pattern, step):
    check_apply(ops, V, D, n, pattern, step)


@pytest.mark.parametrize("D", [4, 64])
def test_apply_on_unaligned_buffers_takes_the_scalar_path(ops, D):
    """the three buffers 4 bytes past a 16-byte boundary: D % 4 == 0 alone does not allow 16-byte accesses"""
    check_apply(ops, 1000, D, 5000, "zipf", 2, guard=65)


@pytest.mark.parametrize("D", [3, 4, 130])
@pytest.mark.parametrize("decoupled", [False, True])
def test_apply_weight_decay_forms_and_grad_scale(ops, D, decoupled):
    hp = dict(HP, weight_decay=0.01, lr=1e-2)
    check_apply(ops, 1000, D, 5000, "zipf", 2, hp=hp, decoupled=decoupled, gs=0.125, seed=1)
    check_apply(ops, 7, D, 17, "zipf", 1000, hp=hp, decoupled=decoupled, gs=0.125, seed=2)


def test_a_reduced_state_is_good_for_one_apply_and_one_table_shape(ops):
    g = torch.Generator().manual_seed(4)
    ids, rows = torch.randint(0, 50, (40,), generator=g).to(DEV), torch.randn(40, 4, generator=g).to(DEV)
    ar = Arena(50, 4, g)
    _, st = reduce_checked(ops, ids, rows, 50, -1)
    with pytest.raises(ValueError):
        ops.row_adam_apply_(*Arena(51, 4, g).pmv, st, 1)
    ops.row_adam_apply_(*ar.pmv, st, 1)
    with pytest.raises(RuntimeError):
        ops.row_adam_apply_(*ar.pmv, st, 1)


# ------------------------------------------------------------------------------------------------ 3. the joint coefficient
def _linked(optim, n_dense, shapes, g, **kw):
    """a dense bucket of n_dense floats and tables of `shapes` on the device -> (flat, tables, FusedAdam, RowSparseAdam)"""
    flat = optim.FlatParams([("w", torch.nn.Parameter((0.1 * torch.randn(n_dense, generator=g)).to(DEV)))])
    tabs = [torch.nn.Parameter((0.1 * torch.randn(V, D, generator=g)).to(DEV)) for V, D in shapes]
    skw = {k: v for k, v in kw.items() if k != "max_grad_norm"}
    opt_s = optim.RowSparseAdam(tabs, **skw)
    return flat, tabs, optim.FusedAdam([flat], **kw).link(opt_s), opt_s


@pytest.mark.parametrize("scale,active", [(1.0, True), (2.0 ** -20, False)])
def test_joint_norm_and_one_coefficient_for_buckets_and_tables(ops, scale, active):
    """a dense bucket of 1000 floats and two tables -- the first receives TWO entries with different padding ids -- through one
    linked step: last_grad_norm within 1 fp32 ulp of the float64 norm over everything (the bound of
    tests/test_optim_clip_gpu.py::test_norm_to_one_ulp: only the final rounding can differ), the coefficient the fp32 formula on
    the device's own norm and exactly 1.0 where the clip is inactive, and both kinds of step taken with that coefficient"""
    from transformers4rec_amd import optim

    gs, max_norm = 0.5, 1.0
    kw = dict(lr=1e-2, weight_decay=0.01, decoupled_weight_decay=True)
    g = torch.Generator().manual_seed(31)
    flat, tabs, opt_d, opt_s = _linked(optim, 1000, [(300, 20), (50, 6)], g, max_grad_norm=max_norm, **kw)
    init = [[t.detach().clone(), torch.zeros_like(t), torch.zeros_like(t)] for t in [flat.data] + [p.data for p in tabs]]
    gd = (scale * spread_rows(1000, 1, g).view(-1)).to(DEV)
    flat.grad.copy_(gd)
    entries = [(0, make_ids("zipf", 300, 400, g)[0], 0), (0, make_ids("zipf", 300, 150, g)[0], -1), (1, make_ids("padmix", 50, 90, g)[0], 0)]
    entries[0][1][::5] = 0
    per_table = {0: [], 1: []}
    for k, ids, pad in entries:
        rows = (scale * spread_rows(ids.numel(), tabs[k].shape[1], g)).to(DEV)
        opt_s.add_rows(tabs[k], ids.to(DEV), rows, padding_idx=pad)
        V = tabs[k].shape[0]
        per_table[k].append((torch.where(ids == pad, torch.full_like(ids, V), ids) if pad >= 0 else ids, rows))
    for p in tabs:
        p._t4r_w_amax = ("stale",)
    opt_d.step(grad_scale=gs)
    torch.cuda.synchronize()
    assert opt_d.step_count == opt_s.step_count == 1 and opt_s._pending == []
    assert not any(hasattr(p, "_t4r_w_amax") for p in tabs)
    # the dense sequence's gradients: each table's entries as ONE list in arrival order, padding mapped to the skipped id V
    cat = {k: (torch.cat([i for i, _ in v]), torch.cat([r for _, r in v])) for k, v in per_table.items()}
    dense_grads = [dense_gradient(ops, p.shape[0], p.shape[1], cat[k][0], cat[k][1], -1) for k, p in enumerate(tabs)]
    want = np.float32(abs(gs) * math.sqrt(sumsq64(gd) + sum(sumsq64(d) for d in dense_grads)))
    out = opt_d._clip_out.cpu()
    d = ulps_apart(out[0], want)
    print(f"joint norm scale={scale}: device {float(out[0])!r} float64 {float(want)!r} ({d} ulp), coef {float(out[1])!r}")
    assert d <= 1 and same_bits(opt_d.last_grad_norm, out[0])
    assert same_bits(out[1], torch.tensor(coef_of(out[0].numpy(), max_norm)))
    assert (float(out[1]) < 1.0) if active else (float(out[1]) == 1.0)
    # both kinds of step with that same coefficient tensor
    coef = opt_d._clip_out[1:].clone()
    hp = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    p, m, v = [t.clone() for t in init[0]]
    ops.adamw_step_(p, gd.clone(), m, v, 1, decoupled=True, grad_scale=gs, zero_grad=False, clip_coef=coef, **hp)
    assert same_bits(flat.data, p) and same_bits(opt_d.state[0][0], m) and same_bits(opt_d.state[0][1], v)
    assert not bool(flat.grad.any())
    for k, tab in enumerate(tabs):
        ids, rows = cat[k]
        wp, wm, wv = dense_sequence(ops, [t.cpu() for t in init[1 + k]], ids, rows.cpu(), -1, 1, hp, True, gs, coef)
        t = touched_rows(ids, tab.shape[0], -1)
        still = torch.ones(tab.shape[0], dtype=torch.bool)
        still[t] = False
        assert 0 < t.numel() < tab.shape[0]
        for got, w, i0 in zip((tab.data, *opt_s.state[k]), (wp, wm, wv), init[1 + k]):
            assert same_bits(got.cpu()[t], w.cpu()[t]) and same_bits(got.cpu()[still], i0.cpu()[still]), k


def test_linked_pair_without_a_clip_is_the_two_objects_stepped_one_after_the_other(ops):
    """link() without max_grad_norm (plain and decoupled): the bits of FusedAdam.step() then RowSparseAdam.step()"""
    from transformers4rec_amd import optim

    for kw in (dict(lr=1e-2, weight_decay=0.01), dict(lr=1e-2, weight_decay=0.01, decoupled_weight_decay=True)):
        runs = []
        for linked in (True, False):
            g = torch.Generator().manual_seed(8)
            flat, tabs, opt_d, opt_s = _linked(optim, 1000, [(300, 20)], g, **kw)
            if not linked:
                opt_s = optim.RowSparseAdam(tabs, **kw)
                opt_d = optim.FusedAdam([flat], **kw)
            for _ in range(2):
                flat.grad.copy_(spread_rows(1000, 1, g).view(-1).to(DEV))
                ids, pad = make_ids("zipf", 300, 400, g)
                opt_s.add_rows(tabs[0], ids.to(DEV), spread_rows(400, 20, g).to(DEV), padding_idx=pad)
                opt_d.step(grad_scale=0.5)
                if not linked:
                    opt_s.step(grad_scale=0.5)
            assert opt_d.last_grad_norm is None and opt_s.step_count == 2
            runs.append([flat.data, tabs[0].data, *opt_d.state[0], *opt_s.state[0]])
        for a, b in zip(*runs):
            assert same_bits(a, b)


def test_the_partial_buffer_grows_with_the_lookups(ops):
    """the tables' partial count depends on n: a later step with more lookups gets a larger buffer, and the norm stays right"""
    from transformers4rec_amd import optim

    g = torch.Generator().manual_seed(9)
    flat, tabs, opt_d, opt_s = _linked(optim, 64, [(1000, 64)], g, max_grad_norm=1.0)
    sizes = []
    for n in (10, 5000, 40):
        gd = spread_rows(64, 1, g).view(-1).to(DEV)
        flat.grad.copy_(gd)
        ids, pad = make_ids("zipf", 1000, n, g)
        rows = spread_rows(n, 64, g)
        opt_s.add_rows(tabs[0], ids.to(DEV), rows.to(DEV), padding_idx=pad)
        opt_d.step()
        sizes.append(opt_d._clip_part.numel())
        want = np.float32(math.sqrt(sumsq64(gd) + sumsq64(dense_gradient(ops, 1000, 64, ids, rows, pad))))
        assert ulps_apart(opt_d.last_grad_norm.cpu(), want) <= 1, n
    assert sizes == [1 + 1, 1 + ops.row_grad_sumsq_parts(5000, 64), 1 + ops.row_grad_sumsq_parts(5000, 64)]


# ------------------------------------------------------------------------------------------------ 4. twenty steps against fp64
def test_twenty_clipped_lazy_steps_against_fp64(ops):
    """V 300, D 20 and a 64-float dense bucket through the linked pair, max_grad_norm 1, a different Zipf subset of 400 lookups
    each step, gradient magnitudes spread over 1e-4 .. 1e2, hyper-parameters rounded to fp32 first; the gradients of steps 2, 7,
    12 and 17 are 2^-24 times smaller, so that the clip is inactive there.  The restatement is tests/row_adam_restatement.py's
    lazy_adam_step with the float64 coefficient folded in (tests/row_clip_restatement.py).  The bound is tests/test_adam_gpu.py's,
    after every step, over the table and the bucket:
        E_dev <= 2 * E_f32 + 4        in units of 2^-24 * (|p_ref| + lr)
    with E_f32 the error of the restatement run in float32 with the fp32 coefficient of the float64 norm."""
    from transformers4rec_amd import optim

    V, D, n, nd, steps, max_norm = 300, 20, 400, 64, 20, 1.0
    hp = dict(lr=f32(1e-2), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8), weight_decay=f32(0.0))
    g = torch.Generator().manual_seed(20)
    p0, d0 = 1e-3 * torch.randn(V, D, generator=g), 1e-3 * torch.randn(nd, generator=g)
    flat = optim.FlatParams([("w", torch.nn.Parameter(d0.clone().to(DEV)))])
    tab = torch.nn.Parameter(p0.clone().to(DEV))
    opt_s = optim.RowSparseAdam([tab], **hp)
    opt_d = optim.FusedAdam([flat], max_grad_norm=max_norm, **hp).link(opt_s)
    r64 = [[p0.double().numpy().copy(), np.zeros((V, D)), np.zeros((V, D))], [d0.double().numpy().copy(), np.zeros(nd), np.zeros(nd)]]
    r32 = [[p0.numpy().copy(), np.zeros((V, D), np.float32), np.zeros((V, D), np.float32)],
           [d0.numpy().copy(), np.zeros(nd, np.float32), np.zeros(nd, np.float32)]]
    rows_out = []
    for step in range(1, steps + 1):
        ids, pad = make_ids("zipf", V, n, g)
        rows = torch.randn(n, D, generator=g) * 10.0 ** (6.0 * torch.rand(n, D, generator=g) - 4.0)
        gd = torch.randn(nd, generator=g) * 10.0 ** (6.0 * torch.rand(nd, generator=g) - 4.0)
        if step % 5 == 2:
            rows, gd = rows * 2.0 ** -24, gd * 2.0 ** -24
        flat.grad.copy_(gd.to(DEV))
        opt_s.add_rows(tab, ids.to(DEV), rows.to(DEV), padding_idx=pad)
        before = tab.detach().cpu().clone()
        opt_d.step()
        norm = rc.joint_norm([gd.numpy()], [(V, ids.numpy(), rows.numpy(), pad)])
        c64, c32 = rc.coef64(norm, max_norm), rc.coef32(norm, max_norm)
        kw = dict(lr=hp["lr"], betas=hp["betas"], eps=hp["eps"])
        t64 = rc.clipped_lazy_adam_step(*r64[0], ids.numpy(), rows.numpy(), step, c64, padding_idx=pad, **kw)
        rc.clipped_lazy_adam_step(*r32[0], ids.numpy(), rows.numpy(), step, c32, padding_idx=pad, **kw)
        rc.clipped_adam_step(*r64[1], gd.numpy(), step, c64, **kw)
        rc.clipped_adam_step(*r32[1], gd.numpy(), step, c32, **kw)
        out = opt_d._clip_out.cpu()
        assert ulps_apart(out[0], np.float32(norm)) <= 1, step
        assert (float(out[1]) == 1.0 and c64 == 1.0) if step % 5 == 2 else (float(out[1]) < 0.1 and c64 < 0.1), (step, float(out[1]), c64)
        t = touched_rows(ids, V, pad)
        assert t.tolist() == t64.tolist() and 0 < t.numel() < V
        still = torch.ones(V, dtype=torch.bool)
        still[t] = False
        assert same_bits(tab.detach().cpu()[still], before[still]), step
        e_dev = max(units(tab.detach().cpu().numpy(), r64[0][0], hp["lr"]), units(flat.data.cpu().numpy(), r64[1][0], hp["lr"]))
        e_f32 = max(units(r32[0][0], r64[0][0], hp["lr"]), units(r32[1][0], r64[1][0], hp["lr"]))
        print(f"clipped row adam step={step}: coef={float(out[1]):.3e} E_dev={e_dev:.2f} E_f32={e_f32:.2f} touched={t.numel()}")
        rows_out.append((step, e_dev, e_f32))
    print(f"clipped row adam: largest E_dev - (2 E_f32 + 4) over {steps} steps: {max(e - (2.0 * f + 4.0) for _, e, f in rows_out):.2f}")
    for step, e_dev, e_f32 in rows_out:
        assert e_dev <= 2.0 * e_f32 + 4.0, (step, e_dev, e_f32)


# ------------------------------------------------------------------------------------------------ 5. whole models
LR = 1e-3
MAX_NORM = 0.01                   # far below the models' first-step norms: the clip is active (asserted)
# as tests/test_row_adam_gpu.py: the GPT-2 position embedding's gradient is summed through fp32 atomics in arrival order, two dense
# runs differ from each other there; a first Adam step from zero moments moves an element by less than lr, so two first steps
# from one start differ by less than 2 lr
ATOMIC_GRADIENT = ("transformer.wpe.weight",)
FIRST_STEP_SPAN = 2.0 * LR


def _build(arch, masking, weight_tying):
    """tests/test_row_adam_gpu.py's small model, copied"""
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


def _train_step(model, batch, opt):
    out = model({"item_id": batch}, training=True)
    out["loss"].backward()
    opt.step()
    torch.cuda.synchronize()
    return float(out["loss"].detach())


@pytest.mark.parametrize("arch,masking", [("gpt2", "clm"), ("xlnet", "mlm")])
def test_whole_model_clipped_first_step_equals_fused_adam_over_both_buckets(arch, masking):
    """One training step from fresh optimizers of a model with an UNTIED sampled head (each table receives one entry), weight
    decay 0, max_grad_norm small enough to clip: the linked pair against FusedAdam(max_grad_norm=same) over both buckets.
    The two norms add the same fp32 values' squares in double in different orders (the dense table bucket with its zero rows
    against the compact rows): within 1 fp32 ulp.  Where the two coefficients are bit-equal every parameter must be (GPT-2's
    position embedding excepted: see ATOMIC_GRADIENT); where they are 1 ulp apart the parameters are held to the 4 units of
    2^-24 (|p| + lr) that tests/test_optim_clip_gpu.py::test_fused_adam_clipped_adamw_on_a_model allows a device step over its
    yardstick -- a first step from zero moments is lr * g / (|g| + eps'), which a relative change of 2^-23 in g moves by less than
    one such unit."""
    from transformers4rec_amd import optim

    model_a, batch = _build(arch, masking, False)
    model_b, _ = _build(arch, masking, False)
    for (_, pa), (_, pb) in zip(model_a.named_parameters(), model_b.named_parameters()):
        assert same_bits(pa, pb)
    dense_a, tables_a = optim.flatten_model(model_a)
    opt_a = optim.FusedAdam([dense_a, tables_a], lr=LR, max_grad_norm=MAX_NORM)
    sparse = dict(optim.row_sparse_tables(model_b))
    assert len(sparse) == 2
    dense_b = optim.FlatParams((n, p) for n, p in model_b.named_parameters() if n not in sparse)
    opt_s = optim.RowSparseAdam(sparse.values(), lr=LR).attach()
    opt_b = optim.FusedAdam([dense_b], lr=LR, max_grad_norm=MAX_NORM).link(opt_s)
    start = {n: p.detach().cpu().clone() for n, p in sparse.items()}
    loss_a, loss_b = _train_step(model_a, batch, opt_a), _train_step(model_b, batch, opt_b)
    opt_s.detach()
    assert loss_a == loss_b and np.isfinite(loss_a)
    assert all(p.grad is None for p in sparse.values())                      # no dense gradient was made for a table
    na, nb = opt_a._clip_out.cpu(), opt_b._clip_out.cpu()
    d = ulps_apart(na[0], nb[0])
    print(f"{arch}: norm dense {float(na[0])!r} linked {float(nb[0])!r} ({d} ulp); coefficient {float(na[1])!r} / {float(nb[1])!r}")
    assert d <= 1 and float(na[1]) < 1.0 and float(nb[1]) < 1.0, "the clip must be active for this test to mean anything"
    pa, pb = dict(model_a.named_parameters()), dict(model_b.named_parameters())
    assert list(pa) == list(pb)
    equal_coef = same_bits(na[1], nb[1])
    print(f"{arch}: the two coefficients are {'bit-equal: every parameter is held to bits' if equal_coef else '1 ulp apart: 4 units'}")
    bad = []
    for n, p in pa.items():
        a, b = p.detach().cpu(), pb[n].detach().cpu()
        assert bool(torch.isfinite(b).all()), n
        if n.endswith(ATOMIC_GRADIENT):
            ok = float((a - b).abs().max()) < FIRST_STEP_SPAN
        elif equal_coef:
            ok = same_bits(a, b)
        else:
            ok = units(b.numpy(), a.numpy(), LR) <= 4.0
        if not ok:
            print(f"{arch}: {n}: max |diff| {float((a - b).abs().max()):.3e}, {int((bits(a) != bits(b)).sum())} of {a.numel()} elements differ")
            bad.append(n)
    assert not bad, bad
    assert all(not same_bits(p, start[n]) for n, p in sparse.items())       # the tables did take their step


# ------------------------------------------------------------------------------------------------ 6. red zones
def _rz_chain(V, D, n, ld, with_coef, decoupled):
    """reduce + coefficient + apply of one table inside the arena: guards round keys, perm, the (pitched) rows, the partials at
    their exact count, the workspace at its exact size, the coefficient and the three table buffers"""
    def fn(a, key):
        lib = rz._lib().load()
        g = rz.gen(V + 3 * D + n)
        ids, pad = make_ids("padmix", V, n, g)
        rows = rz.rn(g, n, D, scale=3.0)
        p0, m0, v0 = rz.rn(g, V, D), 0.1 * rz.rn(g, V, D), 0.01 * rz.rn(g, V, D).abs()
        step, lr, b1, b2, eps, wd, gs, max_norm = 3, 1e-2, 0.9, 0.999, 1e-8, 0.01, 0.5, 0.75
        keys, perm = rz._ops().sort_ids(ids.to(DEV), V, pad)
        K, PM = a.new("keys", "in", rz.I32, n).set(keys), a.new("perm", "in", rz.I32, n).set(perm)
        R = a.new("grad_rows", "in", rz.F32, (n, ld), 0, D).set(rows)
        cnt = lib.t4r_row_grad_sumsq_parts(n, D)
        PART = a.new("part", "out", torch.float64, cnt)
        nb = lib.t4r_row_adam_ws_bytes(n, D)
        WS = a.ws("ws", nb)
        P, M, Vv = (a.new(nm, "inout", rz.F32, (V, D)).set(t) for nm, t in (("param", p0), ("exp_avg", m0), ("exp_avg_sq", v0)))
        assert rz.rc_call(a, "t4r_row_adam_reduce", rz.stream(), V, D, K.ptr, PM.ptr, R.ptr, ld, n, WS.ptr, nb, PART.ptr) == cnt
        sumsq = rz.memo((key, "sumsq"), lambda: torch.tensor([sumsq64(dense_gradient(rz._ops(), V, D, ids, rows, pad))],
                                                             dtype=torch.float64))
        outs = [rz.Out(PART, sumsq, dict(rtol=1e-12, atol=0.0), "sum of the partials in double against the dense gradient's (n * 2^-53)",
                       sel=lambda v: v.sum().view(1))]
        outs[-1].atomic = False
        coef, coef_ptr = 1.0, None
        if with_coef:
            OUT = a.new("out2", "out", rz.F32, 2)
            rz.call(a, "t4r_grad_clip_coef", rz.stream(), PART.ptr, cnt, gs, max_norm, OUT.ptr)
            norm = np.float32(gs * math.sqrt(float(sumsq)))
            coef = float(coef_of(norm, max_norm))
            assert coef < 1.0
            t = "the float64 norm to 1 ulp (section 3), the coefficient from it: 4 ulps of room"
            outs.append(rz.Out(OUT, torch.tensor([float(norm), coef]), dict(rtol=5e-7, atol=0.0), t))
            coef_ptr = OUT.ptr + 4
        rz.call(a, "t4r_row_adam_apply", rz.stream(), P.ptr, M.ptr, Vv.ptr, V, D, n, step, lr, b1, b2, eps, wd, int(decoupled), gs,
                coef_ptr, WS.ptr, nb)

        def ref():
            r = [p0.double().numpy().copy(), m0.double().numpy().copy(), v0.double().numpy().copy()]
            rc.clipped_lazy_adam_step(*r, ids.numpy(), rows.numpy(), step, coef, gs, pad, lr=lr, betas=(b1, b2), eps=eps,
                                      weight_decay=wd, decoupled=decoupled)
            return [torch.from_numpy(x) for x in r]
        rp, rm, rv = rz.memo((key, "adam"), ref)
        t = "test_kernels_gpu.py::test_adam_matches_torch"
        tol = dict(rtol=1e-5, atol=1e-6)
        return outs + [rz.Out(P, rp, tol, t), rz.Out(M, rm, tol, t), rz.Out(Vv, rv, tol, t)]
    return fn


_ROWCLIP = ["t4r_row_adam_reduce", "t4r_grad_clip_coef", "t4r_row_adam_apply"]
REDZONE_CASES = (
    [rz.Case("rowclip", f"clip-{V}x{D}-n{n}-ld{ld}", _ROWCLIP, _rz_chain(V, D, n, ld, True, dec))
     for V, D, n, ld, dec in ((7, 1, 17, 1, True), (50, 3, 300, 5, False), (50, 4, 300, 4, True), (300, 130, 1025, 132, True))]
    + [rz.Case("rowclip", f"nocoef-{V}x{D}-n{n}-ld{ld}", _ROWCLIP[::2], _rz_chain(V, D, n, ld, False, dec))
       for V, D, n, ld, dec in ((50, 4, 300, 7, False), (7, 6, 1, 6, True))]
)
_RZ_BY_ID = {c.id: c for c in REDZONE_CASES}


@pytest.mark.parametrize("cid", list(_RZ_BY_ID))
def test_redzone(cid):
    """the three runs of tests/test_abi_redzone_gpu.py::test_redzone over the launching entries of the tenth header: guards round
    every buffer, the exact partial count and workspace size, both fill bytes, a sibling case in between and a rerun.  No float
    atomics anywhere: every output is bit-identical between the runs."""
    c = _RZ_BY_ID[cid]
    a0, outs0 = rz._run(c, 0x00)
    v0 = rz._values(outs0)
    for o, got in zip(outs0, v0):
        assert bool(torch.isfinite(got).all()), f"{cid}: non-finite value in '{o.buf.name}' under fill 0x00"
        rz._against(o, got, o.ref, f"{cid} fill 0x00")
    del a0
    a1, outs1 = rz._run(c, 0xFF)
    for o, got, first in zip(outs1, rz._values(outs1), v0):
        assert bool(torch.isfinite(got).all()), f"{cid}: non-finite value in '{o.buf.name}' under fill 0xFF"
        assert rz._bits_equal(got, first), f"{cid}: '{o.buf.name}' differs between fill 0x00 and fill 0xFF"
    del a1
    sib = REDZONE_CASES[(REDZONE_CASES.index(c) + 1) % len(REDZONE_CASES)]
    rz._run(sib, 0x00)
    a2, outs2 = rz._run(c, 0x00)
    for o, got, first in zip(outs2, rz._values(outs2), v0):
        assert rz._bits_equal(got, first), f"{cid}: '{o.buf.name}' changed after running {sib.id} in between"
