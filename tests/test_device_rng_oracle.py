"""CPU: the oracle's restatement of the device random streams (oracle/device_rng.py + device_rng.c).
Pinned against the published Philox4x32-10 known-answer vectors (Random123 kat_vectors); numpy form == C form; the
derived rules (threshold, counter layout, MLM selectors) at their edge cases.  The comparison with masks exported from
the device is tests/test_round6_gpu.py (-m gpu)."""
import ctypes

import numpy as np
import pytest
import torch

import device_rng as R
import t4r_oracle as O

KAT = [  # counter[4], key[2], expected[4]  (Random123 kat_vectors: philox4x32 10)
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.fixture(scope="module", autouse=True)
def _c_form():
    import build_c

    build_c.build()
    assert R.use_c()


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    seed, lo, hi = key[0] | (key[1] << 32), ctr[0] | (ctr[1] << 32), ctr[2] | (ctr[3] << 32)
    got = R.philox4x32_10(seed, np.array([lo], dtype=np.uint64), hi)[0]
    assert tuple(int(x) for x in got) == want
    out = (ctypes.c_uint32 * 4)()
    R._load_c().t4r_oracle_philox(seed, lo, hi, out)
    assert tuple(out) == want


def test_numpy_and_c_forms_agree():
    for n in (1, 2, 3, 4, 5, 1023, 100_003):
        for p in (0.1, 0.3, 0.5):
            ctr = R.dropout_ctr_hi(7, 3, R.SITE_FF_ACT)
            assert np.array_equal(R.dropout_keep(2**63 - 5, ctr, n, p), R.dropout_keep(2**63 - 5, ctr, n, p, force_numpy=True))
    for B, L in ((1, 1), (7, 20), (64, 33)):
        a, b = R.mlm_draws(99, 12345, B, L, 0.15), R.mlm_draws(99, 12345, B, L, 0.15, force_numpy=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_threshold_and_counter_layout():
    assert R.keep_threshold(0.0) == 0 and R.keep_threshold(1.0) == 0xFFFFFFFF
    # float32(0.3) * 2^24 = 5033165 exactly (0.3f = 10066330 * 2^-25): keep <=> top 24 bits >= 5033165
    assert R.keep_threshold(0.3) == 5033165 << 8
    assert R.keep_threshold(0.5) == 1 << 31
    assert R.dropout_ctr_hi(1, 255, R.SITE_POS) == (1 << 16) | (255 << 8) | 1
    assert R.dropout_ctr_hi(3, 2, R.SITE_FF_OUT) == (3 << 16) | (2 << 8) | 5
    # prefix property: element idx does not depend on how many elements the site has
    a, b = R.dropout_keep(5, 9, 1000, 0.3), R.dropout_keep(5, 9, 37, 0.3)
    assert np.array_equal(a[:37], b)
    keep = R.dropout_keep(1, R.dropout_ctr_hi(1, 0, 2), 1 << 20, 0.3)
    assert abs(keep.mean() - 0.7) < 2e-3
    # sites / layers / forwards are different streams
    streams = [R.dropout_keep(1, R.dropout_ctr_hi(o, l, s), 4096, 0.3) for o, l, s in ((1, 0, 2), (2, 0, 2), (1, 1, 2), (1, 0, 3))]
    assert all(not np.array_equal(streams[0], s) for s in streams[1:])


def test_mlm_targets_from_device_draws_follow_the_reference_rule():
    """the selector arithmetic (k-th non-pad / labelled position) gives what t4r_oracle.mlm_targets_train gives for the
    same (bern, j1, j2) -- the function the reference fixtures pin -- plus the reference's invariants
    (tests/unit/torch/test_masking.py:117-150): every session with >= 2 items has >= 1 label and < all its items."""
    g = torch.Generator().manual_seed(0)
    B, L = 257, 20
    lens = torch.randint(1, L + 1, (B,), generator=g)
    ids = torch.randint(1, 1000, (B, L), generator=g) * (torch.arange(L)[None] < lens[:, None])
    mask, labels = R.mlm_targets_train_device(ids, seed=4321, offset=3 * B * L, p=0.15)
    bern, u1, u2 = R.mlm_draws(4321, 3 * B * L, B, L, 0.15)
    nonpad = ids != 0
    n_np = nonpad.sum(1)
    k1 = torch.minimum(n_np - 1, (torch.from_numpy(u1) * n_np.float()).long())
    j1 = torch.stack([torch.nonzero(nonpad[b])[k1[b], 0] for b in range(B)])

    def j2_fn(m):
        n = m.sum(1)
        k = torch.minimum(n - 1, (torch.from_numpy(u2) * n.float()).long()).clamp_min(0)
        return torch.stack([torch.nonzero(m[b])[k[b], 0] if n[b] > 0 else torch.tensor(0) for b in range(B)])

    m_ref, lab_ref = O.mlm_targets_train(ids, torch.from_numpy(bern).bool(), j1, j2_fn)
    assert torch.equal(mask, m_ref) and torch.equal(labels, lab_ref)
    multi = lens >= 2
    assert bool((mask.sum(1)[multi] >= 1).all()) and bool((mask.sum(1)[multi] < lens[multi]).all())
    assert bool((mask.sum(1)[~multi] == 0).all())            # a one-item session ends with no label (masking.py:447-457)
    assert torch.equal(labels, torch.where(mask, ids, torch.zeros_like(ids)))


def test_log_uniform_draws_follow_the_reference_distribution():
    """log_uniform_draws restates the device's closed-form draw; here it is held to LogUniformSampler's distribution
    (O.log_uniform_dist) by itself: bin masses of 400 k draws within 5 sigma (the rule of tests/test_kernels_gpu.py:
    test_log_uniform_device_sampler_matches_the_reference_distribution), the range, R = 2, the prefix property."""
    V, n = 100_001, 400_000
    for min_id in (0, 1, 5):
        ids = torch.from_numpy(R.log_uniform_draws(1234, 7, n, min_id, V))
        assert ids.dtype == torch.int64 and ids.shape == (n,)
        assert int(ids.min()) >= min_id and int(ids.max()) < V
        dist = O.log_uniform_dist(V, min_id)
        assert dist.numel() == V and float(dist[:min_id].sum()) == 0.0
        cdf = torch.cat([torch.zeros(1, dtype=torch.float64), dist.double().cumsum(0)])
        edges = torch.unique(torch.logspace(0, 5, 26).long().clamp_(min_id, V))
        for lo, hi in zip(edges[:-1].tolist(), edges[1:].tolist()):
            want = float(cdf[hi] - cdf[lo]) * n
            got = int(((ids >= lo) & (ids < hi)).sum())
            assert abs(got - want) < 5 * (want ** 0.5) + 5, (min_id, lo, hi, got, want)
    # the two smallest ranges: R = 2 has one id; R = 3 has two with masses ln 2 / ln 3 and 1 - ln 2 / ln 3
    for min_id in (0, 1, 5):
        assert np.array_equal(R.log_uniform_draws(99, 3, 4099, min_id, min_id + 1), np.full(4099, min_id))
        two = R.log_uniform_draws(99, 3, 40_000, min_id, min_id + 2)
        assert set(np.unique(two).tolist()) == {min_id, min_id + 1}
        want = 40_000 * np.log(2.0) / np.log(3.0)
        assert abs(int((two == min_id).sum()) - want) < 5 * (want ** 0.5) + 5
    with pytest.raises(ValueError):
        R.log_uniform_draws(99, 3, 4, 5, 5)
    # draw i depends on (seed, position, i) only; other seeds / positions are other streams; min_id only shifts
    a = R.log_uniform_draws(5, 9, 1000, 1, V)
    assert np.array_equal(a[:37], R.log_uniform_draws(5, 9, 37, 1, V))
    assert not np.array_equal(a, R.log_uniform_draws(5, 10, 1000, 1, V))
    assert not np.array_equal(a, R.log_uniform_draws(6, 9, 1000, 1, V))
    assert np.array_equal(a + 4, R.log_uniform_draws(5, 9, 1000, 5, V + 4))


def test_mask_dictionary_shapes():
    m = R.xlnet_dropout_masks(3, 5, 8, 2, 2, 0.3, seed=1, offset=1)
    assert m["input"].shape == (3, 5, 8) and m["pos"].shape == (3, 10, 8) and m["final"].shape == (3, 5, 8)
    assert len(m["layers"]) == 2 and m["layers"][1]["prob"].shape == (3, 2, 5, 5) and m["layers"][0]["ff_act"].shape == (3, 5, 32)
    assert not torch.equal(m["layers"][0]["attn_out"], m["layers"][1]["attn_out"])


@pytest.mark.parametrize("arch", ["gpt2", "bert"])
def test_gpt2_bert_mask_builders(arch):
    """shapes, dtypes, every site == dropout_keep at (offset, MODEL_LEVEL, SITE_INPUT) / (offset, layer, SITE_PROB |
    SITE_ATTN_OUT | SITE_FF_OUT) over the row-major index, BERT's attention rate on the prob site only, and no two sites
    of one forward on one counter."""
    B, L, D, n, NL, seed, offset = 3, 5, 8, 2, 3, 0x1234_5678_9ABC, 7
    ph, pa = (0.3, 0.3) if arch == "gpt2" else (0.1, 0.3)
    if arch == "gpt2":
        m = R.gpt2_dropout_masks(B, L, D, n, NL, ph, seed=seed, offset=offset)
    else:
        m = R.bert_dropout_masks(B, L, D, n, NL, ph, pa, seed=seed, offset=offset)
    assert sorted(m) == ["input", "layers"] and len(m["layers"]) == NL
    want = [("input", m["input"], (B, L, D), R.MODEL_LEVEL, R.SITE_INPUT, ph)]
    for i, lm in enumerate(m["layers"]):
        assert sorted(lm) == ["attn_out", "ff_out", "prob"]
        want += [(f"prob{i}", lm["prob"], (B, n, L, L), i, R.SITE_PROB, pa),
                 (f"attn_out{i}", lm["attn_out"], (B, L, D), i, R.SITE_ATTN_OUT, ph),
                 (f"ff_out{i}", lm["ff_out"], (B, L, D), i, R.SITE_FF_OUT, ph)]
    ctrs = []
    for name, got, shape, layer, site, p in want:
        ctr = (offset << 16) | (layer << 8) | site
        ctrs.append(ctr)
        assert got.dtype == torch.uint8 and tuple(got.shape) == shape, name
        keep = R.dropout_keep(seed, ctr, int(np.prod(shape)), p, force_numpy=True)
        assert np.array_equal(got.numpy().reshape(-1), keep), name
        assert 0 < int(got.sum()) < got.numel(), name
    assert len(set(ctrs)) == len(ctrs) == 1 + 3 * NL
    assert (R.SITE_INPUT, R.SITE_PROB, R.SITE_ATTN_OUT, R.SITE_FF_OUT) == (0, 2, 3, 5) and R.MODEL_LEVEL == 255
    if arch == "bert":          # the two rates are not exchanged: the keep fractions differ (0.9 vs 0.7)
        big = R.bert_dropout_masks(8, 32, 64, 4, 1, 0.1, 0.3, seed=seed, offset=1)
        assert abs(float(big["layers"][0]["prob"].float().mean()) - 0.7) < 0.02
        assert abs(float(big["layers"][0]["attn_out"].float().mean()) - 0.9) < 0.02
        assert abs(float(big["input"].float().mean()) - 0.9) < 0.02
    nxt = (R.gpt2_dropout_masks(B, L, D, n, NL, ph, seed=seed, offset=offset + 1) if arch == "gpt2" else
           R.bert_dropout_masks(B, L, D, n, NL, ph, pa, seed=seed, offset=offset + 1))
    assert not torch.equal(nxt["input"], m["input"]) and not torch.equal(nxt["layers"][0]["prob"], m["layers"][0]["prob"])
