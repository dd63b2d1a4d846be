"""Host half of the sampling heads (Gumbel top-k, replacement-token masking): the restated noise, the second C-ABI header, the
registered operators and the RTD masking module's integer part.  Nothing here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import gumbel_restatement as gr
import transformers4rec_amd as tr
from transformers4rec_amd import _lib, masking, ops, rng, torch_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------- the restatement
def test_uniforms_are_exact_fp32_midpoints_inside_the_open_interval():
    u = gr.uniforms(1234, gr.ctr_hi_of(5), np.arange(37), np.arange(5003))
    assert (u.astype(np.float32).astype(np.float64) == u).all()
    assert u.min() >= 2.0 ** -24 and u.max() <= 1 - 2.0 ** -24
    k = u * 2.0 ** 23 - 0.5
    assert (k == np.floor(k)).all() and k.min() >= 0 and k.max() < 2 ** 23
    g = -np.log(-np.log(np.array([2.0 ** -24, 1 - 2.0 ** -24])))
    assert -2.82 < g[0] < -2.81 and 16.63 < g[1] < 16.64                      # the range the header states


def test_a_draw_depends_on_row_and_item_only():
    seed, c = 77, gr.ctr_hi_of(3)
    whole = gr.uniforms(seed, c, np.arange(12), np.arange(40))
    part = gr.uniforms(seed, c, np.arange(5, 9), np.arange(7, 33, 5))
    assert (part == whole[5:9, 7:33:5]).all()
    assert (gr.uniforms(seed, gr.ctr_hi_of(4), np.arange(12), np.arange(40)) != whole).mean() > 0.99
    assert gr.ctr_hi_of(3) == (3 << 16) | (255 << 8) | 7 and ops.SITE_GUMBEL == gr.SITE_GUMBEL == 7


def test_argmax_frequencies_follow_the_softmax():
    logits = gr.freq_logits()
    g = gr.gumbel(99, gr.ctr_hi_of(1), np.arange(40000), np.arange(61))
    chi2, min_expected = gr.chi2_of_argmax((logits[None, :] + g).argmax(1), logits)
    print(f"chi2 {chi2:.1f} (bound {gr.CHI2_60_Q999}), smallest expected count {min_expected:.1f}")
    assert min_expected >= 5                                                   # Pearson's statistic is usable
    assert chi2 < gr.CHI2_60_Q999


# ---------------------------------------------------------------------------------------------------------- header and ABI
def _decls():
    return re.sub(r"/\*.*?\*/", "", open(_lib.header_path("t4r_hip_sampling.h")).read(), flags=re.S)


def test_second_header_library_and_prototypes_agree():
    lib = _lib.load()
    syms = _lib.header_symbols("t4r_hip_sampling.h")
    assert len(syms) == 6
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/t4r_hip_sampling.h but not exported"
    for name in ("t4r_gumbel_add_f32", "t4r_gumbel_argmax_f32", "t4r_item_sample_f32", "t4r_item_sample_h16"):
        text = open(_lib.header_path("t4r_hip_sampling.h")).read()
        decl = text[: text.index(name + "(void* stream")]
        assert "replaces:" in decl[decl.rindex("/*"):] or "masking.py" in decl[decl.rindex("/*"):], name


def test_no_torch_types_in_the_second_header():
    for word in ("at::", "torch", "Tensor", "std::", "c10"):
        assert word not in _decls(), f"{word} leaked into the C ABI"


def test_argument_errors_come_back_as_messages():
    lib = _lib.load()
    one = ctypes.c_void_p(16)                                                  # non-null, never dereferenced: checks come first
    st = (ctypes.c_long * 8)()
    rc = lib.t4r_item_sample_f32(None, 4, 1000, 8, 1.0, one, 8, one, 8, 257, one, one, one, 1 << 30, None, 0, 1, 2)
    assert rc != 0 and b"1 <= k <= min(256, V)" in lib.t4r_last_error()
    rc = lib.t4r_item_sample_h16(None, 4, 1000, 8, 1.0, one, 8, one, 16, 3, 257, one, one, one, 1 << 30, st, 0, 1, 2)
    assert rc != 0 and b"1 <= k <= min(256, V)" in lib.t4r_last_error()
    rc = lib.t4r_item_sample_f32(None, 4, 100, 8, 1.0, one, 8, one, 8, 101, one, one, one, 1 << 30, None, 0, 1, 2)
    assert rc != 0 and b"item_sample" in lib.t4r_last_error()                  # k > V
    rc = lib.t4r_item_sample_f32(None, 4, 100, 8, 1.0, one, 7, one, 8, 5, one, one, one, 1 << 30, None, 0, 1, 2)
    assert rc != 0 and b"pitch" in lib.t4r_last_error()
    rc = lib.t4r_item_sample_f32(None, 4, 100, 8, 1.0, one, 8, one, 8, 5, one, one, one, 16, None, 0, 1, 2)
    assert rc != 0 and b"workspace" in lib.t4r_last_error()
    rc = lib.t4r_item_sample_h16(None, 4, 100, 8, 1.0, one, 8, ctypes.c_void_p(8), 16, 3, 5, one, one, one, 1 << 30, None, 0, 1, 2)
    assert rc != 0 and b"16-byte aligned" in lib.t4r_last_error()              # the image's alignment
    rc = lib.t4r_gumbel_add_f32(None, one, 4, 100, 99, 0, 1, 1, 2)
    assert rc != 0 and b"gumbel_add: row pitch below V" in lib.t4r_last_error()
    rc = lib.t4r_gumbel_argmax_f32(None, one, 4, 100, 99, 0, 1, 2, one, one)
    assert rc != 0 and b"gumbel_argmax: row pitch below V" in lib.t4r_last_error()
    rc = lib.t4r_gumbel_add_f32(None, one, 4, 100, 100, -1, 1, 1, 2)
    assert rc != 0 and b"rows of the stream" in lib.t4r_last_error()
    rc = lib.t4r_gumbel_add_f32(None, one, 4, 100, 100, 0, 0, 1, 2)
    assert rc != 0 and b"item_stride" in lib.t4r_last_error()
    assert lib.t4r_gumbel_add_f32(None, None, 0, 100, 100, 0, 1, 1, 2) == 0    # nothing to do: no launch, no error


def test_workspace_sizes_are_the_top_k_heads():
    lib = _lib.load()
    for shape in [(1, 7, 8, 7), (12, 5000, 32, 10), (1024, 100001, 128, 20)]:
        assert lib.t4r_item_sample_ws_bytes(*shape) == lib.t4r_item_topk_ws_bytes(*shape) > 0
        assert lib.t4r_item_sample_h16_ws_bytes(*shape) == lib.t4r_item_topk_h16_ws_bytes(*shape) > 0
    assert lib.t4r_item_sample_ws_bytes(0, 7, 8, 7) == 0


def test_every_launching_entry_of_the_second_header_has_a_redzone_case():
    """the completeness check of tests/test_abi_arena_cpu.py, applied to include/t4r_hip_sampling.h and tests/test_sampling_gpu.py"""
    import test_sampling_gpu as sg

    exempt = {"t4r_item_sample_ws_bytes": "size query: nothing launches",
              "t4r_item_sample_h16_ws_bytes": "size query: nothing launches"}
    names = _lib.header_symbols("t4r_hip_sampling.h")
    cased = {e for c in sg.REDZONE_CASES for e in c.entries}
    assert cased <= set(names) and set(exempt) <= set(names)
    missing = [n for n in names if n not in cased and n not in exempt]
    assert not missing, f"entries of include/t4r_hip_sampling.h with neither a red-zone case nor an exemption: {missing}"
    ids = [c.id for c in sg.REDZONE_CASES]
    assert len(ids) == len(set(ids)) == 6


# ---------------------------------------------------------------------------------------------------------- host layer
def test_host_tensors_are_refused():
    x, W = torch.randn(4, 8), torch.randn(50, 8)
    with pytest.raises(_lib.T4RHipError):
        ops.item_sample(x, W, 5, 1, 2)
    with pytest.raises(_lib.T4RHipError):
        ops.gumbel_argmax(torch.randn(4, 9), 1, 2)
    with pytest.raises(_lib.T4RHipError):
        ops.gumbel_add_(torch.randn(4, 9), 1, 2)
    with pytest.raises(_lib.T4RHipError):
        torch.ops.t4r_hip.item_sample(x, W, 1.0, 5, 1, 2, 0)


def test_operators_are_registered_and_their_fakes_give_the_output_shapes():
    assert {"item_sample", "gumbel_argmax"} <= set(torch_ops.OPERATORS)
    schema = str(torch.ops.t4r_hip.item_sample.default._schema)
    assert schema.startswith("t4r_hip::item_sample(Tensor x, Tensor weight, float alpha, "), schema
    x, W = torch.empty(37, 16, device="meta"), torch.empty(1001, 16, device="meta")
    v, i = torch.ops.t4r_hip.item_sample(x, W, 0.5, 20, 1, 2, 0)
    assert v.shape == (37, 20) and v.dtype == torch.float32 and i.shape == (37, 20) and i.dtype == torch.int64
    with FakeTensorMode():
        a, b = torch.empty(5, 16, device="cuda"), torch.empty(300, 16, device="cuda")
        v, i = torch.ops.t4r_hip.item_sample(a, b, 1.0, 7, 1, 2, 0)
        assert v.shape == (5, 7) and i.dtype == torch.int64 and v.device.type == "cuda"
        v, i = torch.ops.t4r_hip.gumbel_argmax(torch.empty(5, 300, device="cuda"), 1, 2, 0)
        assert v.shape == (5,) and i.shape == (5,) and i.dtype == torch.int64


def test_stream_positions_are_part_of_the_rng_state():
    assert "_sample_offset" in rng._STATE_ATTRS
    task = tr.NextItemPredictionTask(weight_tying=True)
    assert task._sample_offset == 0
    torch.manual_seed(5)
    a = task.sample_seed
    task.sample_seed = None
    torch.manual_seed(6)
    assert task.sample_seed != a                                               # lazy default follows torch.manual_seed
    task.sample_seed = 1234
    holder = torch.nn.ModuleDict({"task": task, "m": masking.ReplacementLanguageModeling(8)})
    task._sample_offset, holder["m"]._sample_offset = 9, 4
    st = tr.get_rng_state(holder)
    assert st["task"]["_sample_offset"] == 9 and st["task"]["_sample_seed"] == 1234 and st["m"]["_sample_offset"] == 4
    task._sample_offset, task.sample_seed, holder["m"]._sample_offset = 0, 1, 0
    tr.set_rng_state(holder, st)
    assert (task._sample_offset, task.sample_seed, holder["m"]._sample_offset) == (9, 1234, 4)


# ---------------------------------------------------------------------------------------------------------- RTD masking
def test_rtd_is_registered_under_both_names():
    for name in ("rtd", "replacement"):
        m = masking.parse_masking(name, hidden_size=16, sample_from_batch=True, mlm_probability=0.3)
        assert type(m) is masking.ReplacementLanguageModeling and isinstance(m, masking.MaskedLanguageModeling)
        assert m.sample_from_batch and m.mlm_probability == 0.3 and m.padding_idx == 0 and m.eval_on_last_item_seq_only
    assert tr.ReplacementLanguageModeling is masking.ReplacementLanguageModeling
    assert not masking.ReplacementLanguageModeling(8).sample_from_batch
    with pytest.raises(KeyError, match="rtd, replacement"):
        masking.parse_masking("plm", hidden_size=16)


def _rtd_inputs():
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(1, 50, (4, 9), generator=g)
    ids[0, 6:] = 0
    ids[2, 3:] = 0
    ids[3, 8:] = 0
    labelled = torch.zeros(4, 9, dtype=torch.bool)
    for r, cs in enumerate([(1, 4), (0, 7, 8), (2,), (3, 5, 7)]):
        labelled[r, list(cs)] = True
    target = torch.where(labelled, ids, torch.zeros_like(ids))
    assert bool((target[labelled] != 0).all())
    return ids, target.flatten(), labelled


@pytest.mark.parametrize("from_batch", [False, True])
def test_fake_tokens_integer_part_is_the_references_formula(from_batch):
    ids, target_flat, labelled = _rtd_inputs()
    n = int(labelled.sum())
    originals = target_flat[target_flat != 0]
    g = torch.Generator().manual_seed(8)
    if from_batch:
        drawn = torch.randint(0, n, (n,), generator=g)
        drawn[::2] = torch.arange(n)[::2]                                      # half of the draws pick the row's own label
    else:
        drawn = torch.randint(1, 50, (n,), generator=g)
        drawn[::2] = originals[::2]                                            # updates that partly equal the originals
    m = masking.ReplacementLanguageModeling(8, sample_from_batch=from_batch)
    got = m._replace_tokens(ids, target_flat, drawn)
    want = gr.fake_tokens_formula(ids, target_flat, drawn, 0, from_batch)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert (torch.equal(got[2], want[2]) if from_batch else got[2] == [] == want[2])
    cin, dlab, _ = got
    assert cin.shape == ids.shape and dlab.shape == ids.shape and dlab.dtype == torch.bool
    assert torch.equal(cin[~labelled], ids[~labelled])                         # pads and unlabelled positions untouched
    assert not bool(dlab[~labelled].any())
    assert torch.equal(dlab, cin != ids)                                       # true exactly where the item changed
    assert 0 < int(dlab.sum()) < n                                             # the case holds both kinds


def test_transformer_block_accepts_rtd_where_the_reference_does():
    m = masking.ReplacementLanguageModeling(16)
    tr.TransformerBlock(tr.XLNetConfig.build(16, 2, 1, total_seq_length=20), masking=m)
    tr.TransformerBlock(tr.BertConfig.build(16, 2, 1, total_seq_length=20), masking=m)
    with pytest.raises(ValueError, match="ReplacementLanguageModeling is not supported"):
        tr.TransformerBlock(tr.GPT2Config.build(16, 2, 1, total_seq_length=20), masking=m)


def test_documents_name_the_new_surface():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "t4r_hip_sampling.h" in readme and re.search(r"\b6 (sampling )?entry points", readme)
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "t4r_hip_sampling.h" in integ and "sample_items" in integ and "1e-9" in integ
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "item_sample" in design and "gumbel_noise.h" in design
