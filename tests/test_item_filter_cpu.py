"""Host half of the item filters of the fused top-k / sampling heads: the third C-ABI header, its argument checks, the registered
operators, the task API's host side and the numpy restatement of the contract (tests/item_filter_restatement.py).  Nothing here
needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import item_filter_restatement as fr
import transformers4rec_amd as tr
from transformers4rec_amd import _lib, ops, torch_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = -np.inf


# ---------------------------------------------------------------------------------------------------------- the restatement
def test_restated_bit_words():
    assert [fr.allow_words(V) for V in (0, 1, 64, 65, 128, 129)] == [0, 2, 2, 4, 4, 6]
    allow = np.zeros(70, dtype=np.uint8)
    allow[[0, 31, 32, 63, 64, 69]] = [1, 1, 7, 1, 255, 1]                     # non-zero = allowed
    assert fr.pack_bits(allow).tolist() == [0x80000001, 0x80000001, 0x21, 0]   # item 69 is bit 5 of word 2; pad bits zero
    assert fr.pack_bits(np.ones(33, dtype=bool)).tolist() == [0xFFFFFFFF, 1]


def test_restated_predicate_and_mask():
    allow = np.array([1, 1, 0, 1, 1, 1], dtype=bool)
    excl = np.array([[-1, -1, 0, 0, 4, 6, 99], [-5, -1, -1, -1, -1, -1, -1]])  # pads, a duplicate, ids >= V, a negative id
    ok = fr.allowed(2, 6, allow, excl)
    assert ok.tolist() == [[False, True, False, True, False, True], [True, True, False, True, True, True]]
    assert fr.allowed(2, 6).all() and fr.allowed(2, 6, None, excl)[0].tolist() == [False, True, True, True, False, True]
    s = np.array([[1.0, np.nan, 3.0, np.inf, 5.0, -2.0], [0.5, 0.5, np.nan, 0.5, NINF, 0.25]], dtype=np.float32)
    m = fr.mask(s, ok)
    assert np.isneginf(m[0, [0, 2, 4]]).all() and np.isnan(m[0, 1]) and m[0, 3] == np.inf and m[0, 5] == -2.0
    assert np.isneginf(m[1, 2]) and not np.isnan(m[1]).any()                  # a disallowed NaN becomes -inf
    assert np.isnan(s[1, 2])                                                  # the input is not modified


def test_restated_ranking_and_tail_rule():
    s = np.array([[2.0, 5.0, 5.0, NINF, 1.0], [NINF, NINF, 7.0, NINF, NINF], [NINF] * 5], dtype=np.float32)
    v, i = fr.rank(s, 3)
    assert i.tolist() == [[1, 2, 0], [2, 0, 1], [0, 1, 2]]                     # ties to the lower id, also among -inf
    assert v[0].tolist() == [5.0, 5.0, 2.0]
    v, i = fr.tail(v, i)
    assert i.tolist() == [[1, 2, 0], [2, -1, -1], [-1, -1, -1]]
    assert np.isneginf(v[1, 1:]).all() and np.isneginf(v[2]).all()
    v, i = fr.filtered_topk(s[:1], 2, allow=np.array([1, 0, 1, 1, 1]), excl=np.array([[2]]))
    assert v.tolist() == [[2.0, 1.0]] and i.tolist() == [[0, 4]]


# ---------------------------------------------------------------------------------------------------------- header and ABI
def _decls():
    return re.sub(r"/\*.*?\*/", "", open(_lib.header_path("t4r_hip_filter.h")).read(), flags=re.S)


def test_third_header_library_and_prototypes_agree():
    lib = _lib.load()
    syms = _lib.header_symbols("t4r_hip_filter.h")
    assert len(syms) == 7
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/t4r_hip_filter.h but not exported"
    text = open(_lib.header_path("t4r_hip_filter.h")).read()
    for name in ("t4r_item_allow_pack", "t4r_item_mask_f32", "t4r_item_topk_filtered_f32", "t4r_item_sample_filtered_f32"):
        decl = text[: text.index(name + "(void* stream")]
        comment = decl[decl.rindex("/*"):]
        assert "replaces:" in comment and "prediction_task.py:452-470" in comment and "= -inf" in comment, name
    # the filter tail of every entry that takes one: tests/test_abi_headers_cpu.py


def test_no_torch_types_in_the_third_header():
    for word in ("at::", "torch", "Tensor", "std::", "c10"):
        assert word not in _decls(), f"{word} leaked into the C ABI"


def test_allow_words_table():
    lib = _lib.load()
    for V, want in [(0, 0), (-3, 0), (1, 2), (63, 2), (64, 2), (65, 4), (128, 4), (129, 6), (5003, 158), (100001, 3126)]:
        assert lib.t4r_item_allow_words(V) == want == fr.allow_words(V), V


def test_argument_errors_come_back_as_messages():
    lib = _lib.load()
    one = ctypes.c_void_p(16)                                                  # non-null, never dereferenced: checks come first
    odd = ctypes.c_void_p(18)
    big = 1 << 30

    def f32(name, *tail):
        extra = (0, 1, 2) if "sample" in name else ()
        return getattr(lib, name)(None, 4, 1000, 8, 1.0, one, 8, one, 8, 5, one, one, one, big, None, *extra, *tail)

    def h16(name, *tail):
        extra = (0, 1, 2) if "sample" in name else ()
        return getattr(lib, name)(None, 4, 1000, 8, 1.0, one, 8, one, 16, 3, 5, one, one, one, big, None, *extra, *tail)

    for fn, stem in ((f32, "t4r_item_topk_filtered_f32"), (f32, "t4r_item_sample_filtered_f32"),
                     (h16, "t4r_item_topk_filtered_h16"), (h16, "t4r_item_sample_filtered_h16")):
        tag = stem[4:].replace("_f32", "").encode()
        assert fn(stem, one, one, 1025, 1025) != 0 and b"0 <= n_excl <= 1024" in lib.t4r_last_error()
        assert tag in lib.t4r_last_error()
        assert fn(stem, one, one, -1, 0) != 0 and b"0 <= n_excl <= 1024" in lib.t4r_last_error()
        assert fn(stem, one, one, 20, 19) != 0 and b"ld_excl below n_excl" in lib.t4r_last_error()
        assert fn(stem, one, None, 20, 20) != 0 and b"excl is null with n_excl > 0" in lib.t4r_last_error()
        assert fn(stem, odd, one, 20, 20) != 0 and b"allow_bits must be 4-byte aligned" in lib.t4r_last_error()
    # the unfiltered entries' own checks still come first
    rc = lib.t4r_item_topk_filtered_f32(None, 4, 1000, 8, 1.0, one, 8, one, 8, 257, one, one, one, big, None, None, None, 0, 0)
    assert rc != 0 and b"1 <= k <= min(256, V)" in lib.t4r_last_error()
    rc = lib.t4r_item_topk_filtered_f32(None, 4, 1000, 8, 1.0, one, 8, one, 8, 5, one, one, one, 16, None, None, None, 0, 0)
    assert rc != 0 and b"workspace" in lib.t4r_last_error()
    rc = lib.t4r_item_topk_filtered_h16(None, 4, 1000, 8, 1.0, one, 8, ctypes.c_void_p(8), 16, 3, 5, one, one, one, big, None,
                                        None, None, 0, 0)
    assert rc != 0 and b"16-byte aligned" in lib.t4r_last_error()
    rc = lib.t4r_item_sample_filtered_f32(None, 4, 1000, 8, 1.0, one, 8, one, 8, 5, one, one, one, big, None, -1, 1, 2,
                                          None, None, 0, 0)
    assert rc != 0 and b"row0 must not be negative" in lib.t4r_last_error()
    # the mask and the pack
    assert lib.t4r_item_mask_f32(None, one, 4, 100, 99, 1, one, None, 0, 0) != 0 and b"item_mask: row pitch below V" in lib.t4r_last_error()
    assert lib.t4r_item_mask_f32(None, one, 4, 100, 100, 0, one, None, 0, 0) != 0 and b"item_stride" in lib.t4r_last_error()
    assert lib.t4r_item_mask_f32(None, one, 4, 100, 100, 1, one, one, 1025, 1025) != 0 and b"item_mask: 0 <= n_excl <= 1024" in lib.t4r_last_error()
    assert lib.t4r_item_mask_f32(None, one, 4, 100, 100, 1, odd, None, 0, 0) != 0 and b"4-byte aligned" in lib.t4r_last_error()
    assert lib.t4r_item_mask_f32(None, None, 4, 100, 100, 1, one, None, 0, 0) != 0 and b"item_mask: bad arguments" in lib.t4r_last_error()
    assert lib.t4r_item_allow_pack(None, one, 100, None) != 0 and b"item_allow_pack: bad arguments" in lib.t4r_last_error()
    assert lib.t4r_item_allow_pack(None, one, 100, odd) != 0 and b"4-byte aligned" in lib.t4r_last_error()
    # nothing to do: no launch, no error
    assert lib.t4r_item_mask_f32(None, None, 0, 100, 100, 1, None, None, 0, 0) == 0
    assert lib.t4r_item_allow_pack(None, None, 0, None) == 0
    assert lib.t4r_item_topk_filtered_f32(None, 0, 1000, 8, 1.0, None, 8, None, 8, 5, None, None, None, 0, None, None, None, 0, 0) == 0


def test_every_launching_entry_of_the_third_header_has_a_redzone_case():
    """the completeness check of tests/test_abi_arena_cpu.py, applied to include/t4r_hip_filter.h and tests/test_item_filter_gpu.py"""
    import test_item_filter_gpu as fg

    exempt = {"t4r_item_allow_words": "size query: nothing launches"}
    names = _lib.header_symbols("t4r_hip_filter.h")
    cased = {e for c in fg.REDZONE_CASES for e in c.entries}
    assert set(exempt) <= set(names)
    missing = [n for n in names if n not in cased and n not in exempt]
    assert not missing, f"entries of include/t4r_hip_filter.h with neither a red-zone case nor an exemption: {missing}"
    ids = [c.id for c in fg.REDZONE_CASES]
    assert len(ids) == len(set(ids))


# ---------------------------------------------------------------------------------------------------------- host layer
def test_host_tensors_are_refused():
    x, W = torch.randn(4, 8), torch.randn(50, 8)
    with pytest.raises(_lib.T4RHipError):
        ops.pack_item_filter(torch.ones(50, dtype=torch.bool))
    with pytest.raises(_lib.T4RHipError):
        ops.item_mask_(torch.randn(4, 50), exclude=torch.zeros(4, 2, dtype=torch.int64))
    with pytest.raises(_lib.T4RHipError):
        ops.item_topk(x, W, 5, exclude=torch.zeros(4, 2, dtype=torch.int64))
    with pytest.raises(_lib.T4RHipError):
        ops.item_sample(x, W, 5, 1, 2, allow_bits=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(_lib.T4RHipError):
        torch.ops.t4r_hip.item_topk_filtered(x, W, 1.0, 5, None, torch.zeros(4, 2, dtype=torch.int64))
    with pytest.raises(_lib.T4RHipError):
        torch.ops.t4r_hip.pack_item_filter(torch.ones(50, dtype=torch.bool))
    with pytest.raises(ValueError):
        ops.item_mask_(torch.randn(4, 50), item_stride=0)


def test_operators_are_registered_and_their_fakes_give_the_output_shapes():
    new = {"item_topk_filtered", "item_sample_filtered", "item_mask_", "pack_item_filter"}
    assert new <= set(torch_ops.OPERATORS)
    sch = {n: str(getattr(torch.ops.t4r_hip, n).default._schema) for n in new}
    assert re.match(r"t4r_hip::item_topk_filtered\(Tensor x, Tensor weight, float alpha, (Sym)?[Ii]nt k, Tensor\? allow_bits, "
                    r"Tensor\? exclude\) -> \(Tensor, Tensor\)", sch["item_topk_filtered"]), sch
    assert sch["item_sample_filtered"].startswith("t4r_hip::item_sample_filtered(Tensor x, Tensor weight, float alpha, ")
    assert "Tensor? allow_bits, Tensor? exclude) -> (Tensor, Tensor)" in sch["item_sample_filtered"]
    assert re.match(r"t4r_hip::item_mask_\(Tensor\(a0!\) scores, Tensor\? allow_bits, Tensor\? exclude, (Sym)?[Ii]nt item_stride\) -> \(\)",
                    sch["item_mask_"]), sch                                    # declared as mutating scores
    assert sch["pack_item_filter"] == "t4r_hip::pack_item_filter(Tensor allow) -> Tensor"
    # existing schemas are what they were
    assert re.match(r"t4r_hip::item_topk\(Tensor x, Tensor weight, float alpha, (Sym)?[Ii]nt k\) -> \(Tensor, Tensor\)",
                    str(torch.ops.t4r_hip.item_topk.default._schema))
    with FakeTensorMode():
        a, b = torch.empty(5, 16, device="cuda"), torch.empty(300, 16, device="cuda")
        bits = torch.ops.t4r_hip.pack_item_filter(torch.empty(300, dtype=torch.bool, device="cuda"))
        assert bits.shape == (10,) and bits.dtype == torch.int32 and bits.device.type == "cuda"
        ex = torch.empty(5, 20, dtype=torch.int64, device="cuda")
        v, i = torch.ops.t4r_hip.item_topk_filtered(a, b, 1.0, 7, bits, ex)
        assert v.shape == (5, 7) and v.dtype == torch.float32 and i.shape == (5, 7) and i.dtype == torch.int64
        v, i = torch.ops.t4r_hip.item_sample_filtered(a, b, 1.0, 7, 1, 2, 0, None, ex)
        assert v.shape == (5, 7) and i.dtype == torch.int64 and v.device.type == "cuda"
        s = torch.empty(5, 300, device="cuda")
        assert torch.ops.t4r_hip.item_mask_(s, bits, None, 1) is None


def test_task_api_host_side():
    import inspect

    task = tr.NextItemPredictionTask(weight_tying=True)
    assert task.item_filter_bits is None and "item_filter_bits" not in task.state_dict()
    assert "item_filter_bits" in dict(task.named_buffers(remove_duplicate=False)) or task.item_filter_bits is None
    assert task.set_item_filter(None) is task
    with pytest.raises(RuntimeError, match="not built"):
        task.set_item_filter(torch.ones(5, dtype=torch.bool))
    for fn in (tr.NextItemPredictionTask.forward, tr.NextItemPredictionTask.sample_items):
        p = inspect.signature(fn).parameters["exclude_seen"]
        assert p.default is False
    assert "padding id" in tr.NextItemPredictionTask.forward.__doc__ and "padding id" in tr.NextItemPredictionTask.sample_items.__doc__
    for fn in (ops.item_topk, ops.item_sample):
        ps = inspect.signature(fn).parameters
        assert ps["allow_bits"].kind is ps["exclude"].kind is inspect.Parameter.KEYWORD_ONLY
        assert ps["allow_bits"].default is None and ps["exclude"].default is None


def test_documents_name_the_new_surface():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "t4r_hip_filter.h" in readme and re.search(r"\b7 (filter )?entry points", readme)
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "t4r_hip_filter.h" in integ and "set_item_filter" in integ and "exclude_seen" in integ and "allow_bits" in integ
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "item_filter.h" in design and "itk_collect_filtered" in design and "tail rule" in design
