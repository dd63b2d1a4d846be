"""Item filters of the fused top-k / sampling heads on the GPU (include/t4r_hip_filter.h): the filtered collect epilogues of
csrc/gemm_kernel.h (FEAT bit 5) and csrc/item_topk_h16.hip (EPI 3 / 4), the mask / pack / tail kernels of csrc/item_filter.hip,
ops.item_topk / item_sample with allow_bits / exclude, and the task API (set_item_filter, exclude_seen).

The oracle is independent of the new device code: the EXISTING materialised scores (ops.item_scores, for the sampler followed by
the existing ops.gumbel_add_) are copied to the host and the numpy restatement of the contract (tests/item_filter_restatement.py:
predicate, mask, stable ranking, tail rule) is applied.  Values and ids must be equal bit for bit."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gumbel_restatement as gr
import item_filter_restatement as fr
import test_abi_redzone_gpu as rz

DEV = "cuda"
gpu = pytest.mark.gpu
SEED = 1234
N = 37                       # not a multiple of 32; a row split lands on a row0 that is no multiple of 4
SHAPES = [(5003, 24), (300, 40)]    # V = 5003: M = 1024 sampled items at stride 4; V = 300: M = V, stride 1.  D: padded image rows
TABLES = ["fp32", "fp16", "bf16"]
KS = (1, 10, 70)             # 70 takes t4r_topk's other fallback


def _table(ops, Wd, table):
    return Wd if table == "fp32" else ops.pack_item_table(Wd, table)


@functools.lru_cache(maxsize=None)
def _case(V, D, table):
    """inputs and the two reference score matrices (plain, perturbed) of one shape, computed once by EXISTING entries"""
    from transformers4rec_amd import ops

    g = torch.Generator().manual_seed(V + D)
    x, W = torch.randn((N, D), generator=g), torch.randn((V, D), generator=g)
    xd = x.to(DEV)
    Wt = _table(ops, W.to(DEV), table)
    ctr = gr.ctr_hi_of(3)
    with ops.precision("fp32"):                       # the fp32 table's materialised scores in form 0; an image ignores the mode
        sd = ops.item_scores(xd, Wt, 0.5)
    s = sd.cpu().numpy().copy()
    sn = ops.gumbel_add_(sd.clone(), SEED, ctr).cpu().numpy().copy()
    s.setflags(write=False)
    sn.setflags(write=False)
    return dict(xd=xd, Wt=Wt, s=s, sn=sn, ctr=ctr, sd=sd)


def _dev_filter(ops, allow, excl):
    bits = None if allow is None else ops.pack_item_filter(torch.from_numpy(allow).to(DEV))
    ex = None if excl is None else torch.from_numpy(excl).to(DEV)
    return bits, ex


def _same(got_v, got_i, want_v, want_i, what):
    gv, gi = got_v.cpu().numpy(), got_i.cpu().numpy()
    assert np.array_equal(gi, want_i), f"{what}: ids differ"
    assert np.array_equal(gv.view(np.int32), want_v.view(np.int32)), f"{what}: values differ"


def _no_disallowed(ids, ok, what):
    ids = ids.cpu().numpy()
    r, c = np.nonzero(ids >= 0)
    assert ok[r, ids[r, c]].all(), f"{what}: a disallowed item was returned"


def _lists(V, E, seed):
    """[N, E] exclusion lists in arbitrary order with -1 pads, duplicates, ids >= V and other negative ids"""
    g = np.random.default_rng(seed)
    ex = g.integers(0, V, size=(N, E)).astype(np.int64)
    if E >= 8:
        ex[:, 1] = ex[:, 0]                           # a duplicate
        ex[:, 2] = -1
        ex[::2, 3] = -1
        ex[:, 4] = V
        ex[:, 5] = V + 77
        ex[:, 6] = -9
    return ex


def _filters(V, k, s):
    """(name, allow [V] bool or None, excl [N, E] int64 or None) of the filter cases a .. i of one (shape, k)"""
    g = np.random.default_rng(V * 1000 + k)
    top2k = fr.rank(s, min(2 * k, V))[1]
    out = [("a-all-bits", np.ones(V, dtype=bool), None),
           ("b-p0.5", g.random(V) < 0.5, None),
           ("b-p0.02", g.random(V) < 0.02, None),
           ("c-mod4", np.arange(V) % 4 == 1, None),
           ("e-nothing", np.zeros(V, dtype=bool), None),
           ("g-E0", None, np.zeros((N, 0), dtype=np.int64)),
           ("g-E1", None, top2k[:, :1].copy()),
           ("g-E20", None, np.concatenate([_lists(V, 19, k), top2k[:, :1]], axis=1)),
           ("h-own-topk", None, top2k[:, :k][:, ::-1].copy()),
           ("i-bits-and-list", g.random(V) < 0.5, np.concatenate([_lists(V, 12, k + 1), top2k[:, :k]], axis=1))]
    if k > 3:
        few = np.zeros(V, dtype=bool)
        few[g.choice(V, k - 3, replace=False)] = True
        out.append(("d-k-3-allowed", few, None))
    if k == 1:
        last = np.zeros(V, dtype=bool)
        last[V - 1] = True
        out.append(("f-last-item", last, None))
    return out


# ------------------------------------------------------------------------------------------------ 1. pack and mask
@gpu
@pytest.mark.parametrize("V", [1, 63, 64, 65, 300, 5003])
def test_pack_against_the_restatement(V):
    from transformers4rec_amd import ops

    g = np.random.default_rng(V)
    allow = g.random(V) < 0.4
    allow[-1] = True                                  # the partial last word has a set bit
    ad = torch.from_numpy(allow).to(DEV)
    for a in (ad, ad.to(torch.uint8) * 201):           # bool, and uint8 where any non-zero byte allows
        bits = ops.pack_item_filter(a)
        assert bits.dtype == torch.int32 and bits.shape == (fr.allow_words(V),)
        assert np.array_equal(bits.cpu().numpy().view(np.uint32), fr.pack_bits(allow))      # pad bits are zero


@gpu
@pytest.mark.parametrize("n,V,ld,stride", [(37, 1001, 1004, 1), (5, 333, 340, 3), (17, 300, 300, 1)])
def test_item_mask_touches_only_disallowed_columns(n, V, ld, stride):
    from transformers4rec_amd import ops

    g = np.random.default_rng(n + V)
    pat = g.standard_normal((n, ld)).astype(np.float32)
    pat[:, ::7] = np.nan
    pat[:, 3::11] = np.inf
    pat[:, 5::13] = -np.inf
    items = (V - 1) * stride + 1
    allow = g.random(items) < 0.5
    excl = g.integers(-3, items + 5, size=(n, 9)).astype(np.int64)
    for use_bits, use_list in ((True, True), (True, False), (False, True), (False, False)):
        buf = torch.from_numpy(pat).to(DEV)
        bits, ex = _dev_filter(ops, allow if use_bits else None, excl if use_list else None)
        ret = ops.item_mask_(buf[:, :V], bits, ex, item_stride=stride)
        assert ret.data_ptr() == buf.data_ptr()
        want = pat.copy()
        part = fr.allowed(n, items, allow if use_bits else None, excl if use_list else None)[:, ::stride]
        want[:, :V][~part] = -np.inf
        assert part.shape == (n, V) and (use_bits or use_list) == bool((~part).any())
        # disallowed columns are -inf whatever they held; allowed columns and the pad columns V .. ld - 1 keep the pattern's bits
        assert np.array_equal(buf.cpu().numpy().view(np.int32), want.view(np.int32)), (use_bits, use_list)


# ------------------------------------------------------------------------------------------------ 2. the filtered heads
@gpu
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("V,D", SHAPES)
def test_filtered_topk_equals_the_restatement(V, D, table):
    from transformers4rec_amd import ops

    c = _case(V, D, table)
    for k in KS:
        unf_v, unf_i = ops.item_topk(c["xd"], c["Wt"], k, 0.5)
        unf2_v, unf2_i = ops.item_topk(c["xd"], c["Wt"], min(2 * k, V), 0.5)
        for name, allow, excl in _filters(V, k, c["s"]):
            what = f"item_topk {table} V={V} k={k} {name}"
            bits, ex = _dev_filter(ops, allow, excl)
            v, i = ops.item_topk(c["xd"], c["Wt"], k, 0.5, allow_bits=bits, exclude=ex)
            st = ops.item_topk_stats()
            wv, wi = fr.filtered_topk(c["s"], k, allow, excl)
            _same(v, i, wv, wi, what)
            _no_disallowed(i, fr.allowed(N, V, allow, excl), what)
            # the on-device composition over the same scores
            with ops.precision("fp32"):
                m = ops.item_mask_(ops.item_scores(c["xd"], c["Wt"], 0.5).clone(), bits, ex)
            cv, ci = ops.topk(m, k)
            _same(cv, ci.masked_fill(cv == float("-inf"), -1), wv, wi, what + " (composition)")
            if name == "a-all-bits":
                assert torch.equal(v, unf_v) and torch.equal(i, unf_i), what + ": != the unfiltered head"
            if name == "c-mod4" and V == 5003:
                # no sampled item (0, 4, 8, ...) is allowed: the threshold is -inf, all V / 4 allowed items fit the list
                assert st["fallback_rows"] == 0, (what, st)
            if name == "d-k-3-allowed":
                assert (i[:, k - 3:] == -1).all() and torch.isneginf(v[:, k - 3:]).all() and (i[:, :k - 3] >= 0).all(), what
            if name == "e-nothing":
                assert (i == -1).all() and torch.isneginf(v).all(), what
            if name == "f-last-item":
                assert (i == V - 1).all(), what
            if name == "h-own-topk" and 2 * k <= V:
                assert torch.equal(v, unf2_v[:, k:]) and torch.equal(i, unf2_i[:, k:]), what + ": != entries k .. 2k-1 of item_topk(2k)"


@gpu
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("V,D", SHAPES)
def test_filtered_sample_equals_the_restatement(V, D, table):
    from transformers4rec_amd import ops

    c = _case(V, D, table)
    for k in KS:
        for name, allow, excl in _filters(V, k, c["sn"]):
            what = f"item_sample {table} V={V} k={k} {name}"
            bits, ex = _dev_filter(ops, allow, excl)
            v, i = ops.item_sample(c["xd"], c["Wt"], k, SEED, c["ctr"], 0.5, allow_bits=bits, exclude=ex)
            wv, wi = fr.filtered_topk(c["sn"], k, allow, excl)
            _same(v, i, wv, wi, what)
            _no_disallowed(i, fr.allowed(N, V, allow, excl), what)
            if name == "a-all-bits":
                uv, ui = ops.item_sample(c["xd"], c["Wt"], k, SEED, c["ctr"], 0.5)
                assert torch.equal(v, uv) and torch.equal(i, ui), what + ": != the unfiltered sampler"


@gpu
@pytest.mark.parametrize("table", ["fp32", "fp16"])
def test_row_split_invariance(table):
    from transformers4rec_amd import ops

    V, D, k = SHAPES[0][0], SHAPES[0][1], 10
    c = _case(V, D, table)
    allow = np.arange(V) % 3 != 0
    excl = np.concatenate([_lists(V, 12, 5), fr.rank(c["sn"], 4)[1]], axis=1)
    bits, ex = _dev_filter(ops, allow, excl)
    v, i = ops.item_sample(c["xd"], c["Wt"], k, SEED, c["ctr"], 0.5, allow_bits=bits, exclude=ex)
    a, b = 5, 22
    pv, pi = ops.item_sample(c["xd"][a:b], c["Wt"], k, SEED, c["ctr"], 0.5, row0=a, allow_bits=bits, exclude=ex[a:b])
    assert torch.equal(pv, v[a:b]) and torch.equal(pi, i[a:b])
    tv, ti = ops.item_topk(c["xd"], c["Wt"], k, 0.5, allow_bits=bits, exclude=ex)
    qv, qi = ops.item_topk(c["xd"][a:b], c["Wt"], k, 0.5, allow_bits=bits, exclude=ex[a:b])
    assert torch.equal(qv, tv[a:b]) and torch.equal(qi, ti[a:b])


# ------------------------------------------------------------------------------------------------ 3. overflow
@gpu
@pytest.mark.parametrize("table", ["fp32", "bf16"])
@pytest.mark.parametrize("noisy", [False, True])
def test_overflow_rows_are_exact_under_a_filter(table, noisy):
    """the adversarial table of tests/test_sampling_gpu.py::test_overflow_rows_take_the_materialised_path: 3000 copies of the best
    item overflow the lists of six rows; under a filter the materialised path must mask too"""
    from transformers4rec_amd import ops

    n, V, D, k = 12, 5000, 32, 10
    g = torch.Generator().manual_seed(13)
    x, W = torch.randn((n, D), generator=g), torch.randn((V, D), generator=g)
    best = 2.0 * W[17]
    big = [0, 1, 2, 5, 9, 10]
    x[big] = best * 2.0 ** 25
    sel = torch.randperm(V, generator=torch.Generator().manual_seed(7))[:3000]
    W[sel] = best
    xd = x.to(DEV)
    Wt = _table(ops, W.to(DEV), table)
    ctr = gr.ctr_hi_of(4)
    with ops.precision("fp32"):
        sd = ops.item_scores(xd, Wt).clone()
    if noisy:
        ops.gumbel_add_(sd, SEED, ctr)
    s = sd.cpu().numpy()
    gnp = np.random.default_rng(3)
    allow = gnp.random(V) < 0.9                        # ~2700 allowed copies: still beyond the list of a row
    lowest = np.sort(sel.numpy())[:4]
    excl = np.tile(lowest[None, :], (n, 1)).astype(np.int64)                  # the four copies that would win the ties
    bits, ex = _dev_filter(ops, allow, excl)
    if noisy:
        v, i = ops.item_sample(xd, Wt, k, SEED, ctr, allow_bits=bits, exclude=ex)
    else:
        v, i = ops.item_topk(xd, Wt, k, allow_bits=bits, exclude=ex)
    st = ops.item_topk_stats()
    print(f"[filtered overflow {table} noisy={noisy}] fallback rows {st['fallback_rows']} of {n} (cap {st['list_capacity']})")
    # which rows must take the materialised path follows from the scores alone (csrc/item_topk.hip, steps 1, 2 and 4): the
    # threshold is the k-th best ALLOWED score of the strided sample, a row overflows when more allowed scores than its list
    # holds reach it.  Nothing else may fall back: the filter itself overflows no list.
    ok = fr.allowed(n, V, allow, excl)
    ms = fr.mask(s, ok)
    M, cap = st["sample_rows"], st["list_capacity"]
    stride = V // M if M < V else 1
    t0 = np.sort(ms[:, :(M - 1) * stride + 1:stride], axis=1)[:, -k]
    cand = ((ms >= t0[:, None]) & ok).sum(1)
    flagged = (cand > cap) | (cand < k)
    assert flagged[big].all() and int(flagged.sum()) >= 6
    assert st["fallback_rows"] == int(flagged.sum())
    wv, wi = fr.filtered_topk(s, k, allow, excl)
    _same(v, i, wv, wi, f"overflow {table} noisy={noisy}")
    _no_disallowed(i, ok, "overflow")
    assert not set(i[big].flatten().tolist()) & set(lowest.tolist())


# ------------------------------------------------------------------------------------------------ 4. the task
def _tiny_model(V=3001, L=20, D=64):
    import transformers4rec_amd as tr

    schema = tr.session_schema(V - 1, L)
    torch.manual_seed(0)
    inputs = tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=L, masking="mlm", embedding_dim_default=D)
    cfg = tr.XLNetConfig.build(D, 4, 1, total_seq_length=L, dropout=0.0)
    model = cfg.to_torch_model(inputs, tr.NextItemPredictionTask(weight_tying=True, softmax_temperature=2.0))
    return model.to(DEV).eval(), schema


def _hidden(model, ids):
    cap = {}
    h = model.transformer_block.register_forward_hook(lambda m, i, o: cap.__setitem__("hid", o))
    with torch.no_grad():
        out = model({"item_id": ids})
    h.remove()
    hid = cap["hid"]
    return out, (hid[0] if isinstance(hid, (tuple, list)) else hid)


@gpu
def test_task_routes_apply_the_filter():
    import transformers4rec_amd as tr
    from transformers4rec_amd import ops

    B, L, k = 24, 20, 5
    model, schema = _tiny_model()
    task = model.prediction_task
    V = task.pre.module.output_weights.shape[0]
    ids = tr.random_data_from_schema(schema, B, L, seed=4)["item_id"].to(DEV)
    _, hid = _hidden(model, ids)
    seen = ids.cpu().numpy().astype(np.int64)
    allow = np.random.default_rng(0).random(V) < 0.5

    def run(**kw):
        with torch.no_grad(), ops.precision("fp32"):
            return task(hid, **kw)

    plain = run()
    plain_k = {m: (task.set_topk_mode(m), run(top_k=k))[1] for m in ("fused", "materialize")}
    assert "item_filter_bits" not in task.state_dict()
    for with_bits in (False, True):
        task.set_item_filter(torch.from_numpy(allow) if with_bits else None)
        assert (task.item_filter_bits is not None) == with_bits and "item_filter_bits" not in task.state_dict()
        al = allow if with_bits else None
        ok = fr.allowed(B, V, al, seen)
        full = run(exclude_seen=True)                                         # top_k=None: the masked scores
        want_full = fr.mask(plain.cpu().numpy(), ok)
        assert np.array_equal(full.cpu().numpy().view(np.int32), want_full.view(np.int32))
        wv, wi = fr.tail(*fr.rank(want_full, k))
        for mode in ("fused", "materialize"):
            task.set_topk_mode(mode)
            calls = ops.item_topk_stats()["calls"]
            v, i = run(top_k=k, exclude_seen=True)
            assert (ops.item_topk_stats()["calls"] == calls + 1) == (mode == "fused")
            _same(v, i, wv, wi, f"task {mode} bits={with_bits}")
            for r in range(B):
                assert not set(i[r].tolist()) & set(seen[r].tolist()), (mode, r)         # disjoint from the session (and the pad id)
            if with_bits:                                                     # the catalogue filter alone, no exclude_seen
                v, i = run(top_k=k)
                _same(v, i, *fr.filtered_topk(plain.cpu().numpy(), k, al, None), f"task {mode} bits only")
        # the serving image: its own scores, masked
        task.prepare_serving("fp16")
        xr, inv_t = task._inference_rows(hid.float())
        s16 = ops.item_scores(xr, task._serving_weights(), inv_t).cpu().numpy()
        h16 = ops.item_topk_stats()["calls_h16"]
        v, i = run(top_k=k, exclude_seen=True)
        assert ops.item_topk_stats()["calls_h16"] == h16 + 1
        _same(v, i, *fr.filtered_topk(s16, k, al, seen), f"task serving bits={with_bits}")
        assert np.array_equal(run(exclude_seen=True).cpu().numpy().view(np.int32), fr.mask(s16, ok).view(np.int32))
        task.drop_serving_image()
    # no filter, no flag: what it was
    task.set_item_filter(None)
    assert torch.equal(run(), plain) and torch.equal(run(exclude_seen=False), plain)
    for mode in ("fused", "materialize"):
        task.set_topk_mode(mode)
        v, i = run(top_k=k, exclude_seen=False)
        assert torch.equal(v, plain_k[mode][0]) and torch.equal(i, plain_k[mode][1])
    # the model passes the flag through
    model.top_k, model.exclude_seen = k, True
    with torch.no_grad(), ops.precision("fp32"):
        mv, mi = model({"item_id": ids})
    _same(mv, mi, *fr.filtered_topk(plain.cpu().numpy(), k, None, seen), "model")


@gpu
def test_task_sample_items_excludes_seen_and_replays():
    import transformers4rec_amd as tr
    from transformers4rec_amd import ops

    B, L, k = 24, 20, 4
    model, schema = _tiny_model()
    task = model.prediction_task
    ids = tr.random_data_from_schema(schema, B, L, seed=4)["item_id"].to(DEV)
    _, hid = _hidden(model, ids)
    task.sample_seed = 4321
    state = tr.get_rng_state(model)
    v, i = task.sample_items(hid, k=k, exclude_seen=True)
    for r in range(B):
        assert not set(i[r].tolist()) & set(ids[r].tolist())
    xr, inv_t = task._inference_rows(hid.float())
    W = task.pre.module.output_weights.detach()
    with ops.precision("fp32"):
        sn = ops.gumbel_add_(ops.item_scores(xr, W, inv_t).clone(), 4321, gr.ctr_hi_of(1)).cpu().numpy()
    _same(v, i, *fr.filtered_topk(sn, k, None, ids.cpu().numpy()), "sample_items")
    v2, i2 = task.sample_items(hid, k=k, exclude_seen=True)
    assert not torch.equal(i, i2)                                             # the stream advances
    tr.set_rng_state(model, state)
    v3, i3 = task.sample_items(hid, k=k, exclude_seen=True)
    assert torch.equal(v3, v) and torch.equal(i3, i)                          # ... and replays
    tr.set_rng_state(model, state)
    uv, ui = task.sample_items(hid, k=k)                                      # without the flag: the unfiltered draw
    rv, ri = ops.item_sample(xr, W, k, 4321, gr.ctr_hi_of(1), inv_t)
    assert torch.equal(uv, rv) and torch.equal(ui, ri)


@gpu
def test_operators_equal_the_functions():
    from transformers4rec_amd import ops, torch_ops  # noqa: F401

    (V, D), k = SHAPES[1], 7
    c = _case(V, D, "fp32")
    allow = np.arange(V) % 2 == 0
    excl = _lists(V, 9, 2)
    bits, ex = _dev_filter(ops, allow, excl)
    assert torch.equal(torch.ops.t4r_hip.pack_item_filter(torch.from_numpy(allow).to(DEV)), bits)
    v, i = ops.item_topk(c["xd"], c["Wt"], k, 0.5, allow_bits=bits, exclude=ex)
    ov, oi = torch.ops.t4r_hip.item_topk_filtered(c["xd"], c["Wt"], 0.5, k, bits, ex)
    assert torch.equal(v, ov) and torch.equal(i, oi)
    v, i = ops.item_sample(c["xd"], c["Wt"], k, SEED, c["ctr"], 0.5, 3, allow_bits=bits, exclude=ex)
    ov, oi = torch.ops.t4r_hip.item_sample_filtered(c["xd"], c["Wt"], 0.5, k, SEED, c["ctr"], 3, bits, ex)
    assert torch.equal(v, ov) and torch.equal(i, oi)
    a, b = c["sd"].clone(), c["sd"].clone()
    ops.item_mask_(a, bits, ex)
    assert torch.ops.t4r_hip.item_mask_(b, bits, ex, 1) is None
    assert torch.equal(a, b) and bool(torch.isneginf(a).any())


# ------------------------------------------------------------------------------------------------ 5. red zones and poison
def _rz_filter(a, g, n, items, E, ld_excl):
    """the filter's buffers with guards: the allow bytes, the bit words at their exact size (packed by t4r_item_allow_pack in
    the arena) and the sorted lists in a pitched window (ld_excl > E); returns (BITS, EX, numpy allow, numpy lists)"""
    lib = rz._lib().load()
    allow = (torch.rand(items, generator=g) < 0.6).numpy()
    ex = torch.randint(-2, items + 3, (n, E), generator=g)
    ex[:, 0] = -1
    ex = torch.sort(ex, dim=1).values                  # the C ABI takes sorted rows
    AL = a.new("allow", "in", rz.U8, items).set(torch.from_numpy(allow).to(torch.uint8) * 3)
    BITS = a.new("allow_bits", "out", rz.I32, lib.t4r_item_allow_words(items))
    EX = a.new("excl", "in", rz.I64, (n, ld_excl), 0, E).set(ex)
    rz.call(a, "t4r_item_allow_pack", rz.stream(), AL.ptr, items, BITS.ptr)
    return BITS, EX, allow, ex.numpy()


def _rz_mask(n, V, ld, stride, with_bits):
    def fn(a, key):
        g = rz.gen(n + V + stride)
        s = rz.dy(g, n, V)
        items = (V - 1) * stride + 1
        S = a.new("scores", "inout", rz.F32, (n, ld), 0, V).set(s)
        E = 6
        BITS, EX, allow, ex = _rz_filter(a, g, n, items, E, E + 3)
        rz.call(a, "t4r_item_mask_f32", rz.stream(), S.ptr, n, V, ld, stride, BITS.ptr if with_bits else None, EX.ptr, E, E + 3)
        ok = fr.allowed(n, items, allow if with_bits else None, ex)[:, ::stride]
        t = "tests/item_filter_restatement.py (exact)"
        return [rz.Out(S, torch.from_numpy(fr.mask(s.numpy(), ok)), None, t),
                rz.Out(BITS, torch.from_numpy(fr.pack_bits(allow).view(np.int32)), None, t)]
    return fn


def _rz_head(n, V, D, k, table, noisy, row0):
    """a filtered entry with its exact workspace against the composition built in the same arena from the unfiltered entries,
    t4r_item_mask_f32 and t4r_topk"""
    def fn(a, key):
        from transformers4rec_amd import ops

        lib = rz._lib().load()
        ctr = gr.ctr_hi_of(9)
        g = rz.gen(n * 3 + V + D)
        x, W = rz.dy(g, n, D), rz.dy(g, V, D)
        alpha = 0.5
        ldx, ldw, ldc = D + 4, D + 4, (V + 3) // 4 * 4 + 4
        X, Wb = a.new("X", "in", rz.F32, (n, ldx), 0, D).set(x), a.new("W", "in", rz.F32, (V, ldw), 0, D).set(W)
        OV, OI = a.new("out_val", "out", rz.F32, (n, k)), a.new("out_idx", "out", rz.I64, (n, k))
        C = a.new("C", "out", rz.F32, (n, ldc), 0, V)
        TV, TI = a.new("topk_val", "out", rz.F32, (n, k)), a.new("topk_idx", "out", rz.I64, (n, k))
        E = 5
        BITS, EX, allow, ex = _rz_filter(a, g, n, V, E, E + 2)
        filt = (BITS.ptr, EX.ptr, E, E + 2)
        st = (ctypes.c_long * 8)()
        stp = ctypes.cast(st, ctypes.c_void_p)
        tail = (row0, SEED, ctr) if noisy else ()
        stem = "t4r_item_sample" if noisy else "t4r_item_topk"
        if table == "fp32":
            nb = getattr(lib, stem + "_ws_bytes")(n, V, D, k)
            WS = a.ws("workspace", nb)
            rz.call(a, stem + "_filtered_f32", rz.stream(), n, V, D, alpha, X.ptr, ldx, Wb.ptr, ldw, k, OV.ptr, OI.ptr, WS.ptr, nb,
                    stp, *tail, *filt)
            with ops.precision("fp32"):
                ops.gemm(X.win, Wb.win, False, True, alpha=alpha, out=C.win)
        else:
            td, code = (torch.float16, 3) if table == "fp16" else (torch.bfloat16, 2)
            ild = lib.t4r_item_table_image_ld(D)
            ldp = ild + 8
            IM = a.new("image", "out", td, (V, ldp), 0, D).allow(D, ldp)
            WS1 = a.ws("scores_ws", n * ild * 2)
            nb = getattr(lib, stem + "_h16_ws_bytes")(n, V, D, k)
            WS = a.ws("workspace", nb)
            rz.call(a, "t4r_item_table_pack_h16", rz.stream(), Wb.ptr, ldw, V, D, code, IM.ptr, ldp)
            rz.call(a, stem + "_filtered_h16", rz.stream(), n, V, D, alpha, X.ptr, ldx, IM.ptr, ldp, code, k, OV.ptr, OI.ptr, WS.ptr,
                    nb, stp, *tail, *filt)
            rz.call(a, "t4r_item_scores_h16", rz.stream(), n, V, D, alpha, X.ptr, ldx, IM.ptr, ldp, code, C.ptr, ldc, WS1.ptr,
                    n * ild * 2)
        if noisy:
            rz.call(a, "t4r_gumbel_add_f32", rz.stream(), C.ptr, n, V, ldc, row0, 1, SEED, ctr)
        rz.call(a, "t4r_item_mask_f32", rz.stream(), C.ptr, n, V, ldc, 1, *filt)
        rz.call(a, "t4r_topk", rz.stream(), C.ptr, n, V, ldc, k, TV.ptr, TI.ptr)
        torch.cuda.synchronize()
        assert torch.equal(OV.win, TV.win), "filtered head != topk(item_mask(scores), k): values"
        assert torch.equal(OI.win, TI.win.masked_fill(TV.win == float("-inf"), -1)), "filtered head != topk(item_mask(scores), k): ids"
        ok = fr.allowed(n, V, allow, ex)
        ids = OI.win.cpu().numpy()
        r, c = np.nonzero(ids >= 0)
        assert ok[r, ids[r, c]].all(), "a disallowed item was returned"
        if noisy:
            return [rz.Out(OV), rz.Out(OI)]
        # exact inputs (multiples of 1/8): the fp32 scores are exact, the restatement gives the bits
        S = rz.memo((key, "S"), lambda: (alpha * x.double() @ W.double().t()).float().numpy())
        wv, wi = fr.filtered_topk(S, k, allow, ex)
        t = "tests/item_filter_restatement.py (bit for bit; exact inputs)"
        return [rz.Out(OV, torch.from_numpy(wv), None, t), rz.Out(OI, torch.from_numpy(wi), None, t)]
    return fn


_PM = ["t4r_item_allow_pack", "t4r_item_mask_f32"]
REDZONE_CASES = [
    rz.Case("filter", "item_mask-7-1001-stride3", _PM, _rz_mask(7, 1001, 1004, 3, True)),
    rz.Case("filter", "item_mask-33-333-list-only", _PM, _rz_mask(33, 333, 333, 1, False)),
    rz.Case("filter", "item_topk_filtered_f32-33-129-20-k20", _PM + ["t4r_item_topk_filtered_f32"],
            _rz_head(33, 129, 20, 20, "fp32", False, 0)),
    rz.Case("filter", "item_sample_filtered_f32-33-1000-8-k5", _PM + ["t4r_item_sample_filtered_f32"],
            _rz_head(33, 1000, 8, 5, "fp32", True, 5)),
    rz.Case("filter", "item_topk_filtered_h16-fp16-33-1000-40-k10", _PM + ["t4r_item_topk_filtered_h16"],
            _rz_head(33, 1000, 40, 10, "fp16", False, 0)),
    rz.Case("filter", "item_sample_filtered_h16-bf16-9-300-24-k7", _PM + ["t4r_item_sample_filtered_h16"],
            _rz_head(9, 300, 24, 7, "bf16", True, 3)),
]
_RZ_BY_ID = {c.id: c for c in REDZONE_CASES}


@gpu
@pytest.mark.parametrize("cid", list(_RZ_BY_ID))
def test_redzone(cid):
    """the three runs of tests/test_abi_redzone_gpu.py::test_redzone over the entries of the third header: guards round every
    buffer (the bit array and the lists included), exact workspaces, both fill bytes, a sibling case in between and a rerun.
    -inf is a legitimate output here (masked scores, short rows); NaN is not."""
    c = _RZ_BY_ID[cid]
    a0, outs0 = rz._run(c, 0x00)
    v0 = rz._values(outs0)
    for o, got in zip(outs0, v0):
        if got.dtype.is_floating_point:
            assert not bool(torch.isnan(got).any()), f"{cid}: NaN in '{o.buf.name}' under fill 0x00"
        if o.ref is not None:
            rz._against(o, got, o.ref, f"{cid} fill 0x00")
    del a0
    a1, outs1 = rz._run(c, 0xFF)
    for o, got, first in zip(outs1, rz._values(outs1), v0):
        if got.dtype.is_floating_point:
            assert not bool(torch.isnan(got).any()), f"{cid}: NaN in '{o.buf.name}' under fill 0xFF"
        assert rz._bits_equal(got, first), f"{cid}: '{o.buf.name}' differs between fill 0x00 and fill 0xFF"
    del a1
    sib = REDZONE_CASES[(REDZONE_CASES.index(c) + 1) % len(REDZONE_CASES)]
    rz._run(sib, 0x00)
    a2, outs2 = rz._run(c, 0x00)
    for o, got, first in zip(outs2, rz._values(outs2), v0):
        assert rz._bits_equal(got, first), f"{cid}: '{o.buf.name}' changed after running {sib.id} in between"
