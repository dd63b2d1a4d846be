"""Host half of the fused top-k inference head: the C ABI carries the two entry points, the host layer refuses host
tensors, the task's topk_mode resolves by the rule of size_head_mode, and the registered operator propagates under
fake tensors.  Nothing here needs a GPU."""
import os
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import transformers4rec_amd as tr
from transformers4rec_amd import _lib, ops, torch_ops


def test_library_exports_and_header_declares_the_entry_points():
    lib = _lib.load()
    syms = _lib.header_symbols()
    for name in ("t4r_item_topk_f32", "t4r_item_topk_ws_bytes"):
        assert name in syms and hasattr(lib, name) and name in _lib.signatures()
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    decl = text[: text.index("t4r_item_topk_ws_bytes(int")]
    comment = decl[decl.rindex("/*"):]
    assert "prediction_task.py" in comment and "torch.topk" in comment         # the reference lines it replaces


def test_workspace_is_far_below_the_score_matrix():
    lib = _lib.load()
    for N, V, D, k in [(1024, 100001, 128, 20), (1024, 1000001, 256, 100), (256, 10000001, 512, 10)]:
        ws = lib.t4r_item_topk_ws_bytes(N, V, D, k)
        assert 0 < ws < 4 * N * ops.pad_ld(V) / 8, (N, V, D, k, ws)
    assert lib.t4r_item_topk_ws_bytes(1, 7, 8, 7) > 0
    assert lib.t4r_item_topk_ws_bytes(0, 7, 8, 7) == 0


def test_workspace_sizes_are_the_recorded_ones():
    """(N, V, D, k) -> bytes, as the build before the two heads got one driver returned them: the plan did not move"""
    ws = _lib.load().t4r_item_topk_ws_bytes
    for shape, b in [((1, 7, 8, 7), 1536), ((12, 5000, 32, 10), 378624), ((37, 4099, 100, 1), 1168640),
                     ((1024, 100001, 128, 20), 35610880), ((1024, 1000001, 256, 100), 261939456),
                     ((256, 10000001, 512, 10), 132242432)]:
        assert ws(*shape) == b, (shape, ws(*shape), b)


def test_argument_errors_come_back_as_messages():
    lib = _lib.load()
    rc = lib.t4r_item_topk_f32(None, 4, 100, 8, 1.0, None, 8, None, 8, 10, None, None, None, 0, None)
    assert rc != 0 and b"item_topk" in lib.t4r_last_error()


def test_host_tensors_are_refused():
    x, W = torch.randn(4, 8), torch.randn(50, 8)
    with pytest.raises(_lib.T4RHipError):
        ops.item_topk(x, W, 5)
    with pytest.raises(_lib.T4RHipError):
        torch.ops.t4r_hip.item_topk(x, W, 1.0, 5)
    st = ops.item_topk_stats()
    assert {"calls", "fallback_rows"} <= set(st)


def test_topk_mode_validation_and_auto_rule(monkeypatch):
    P = tr.NextItemPredictionTask
    with pytest.raises(ValueError):
        P(weight_tying=True, topk_mode="recompute")
    task = P(weight_tying=True)
    assert task.topk_mode == "auto"
    with pytest.raises(ValueError):
        task.set_topk_mode("nope")
    monkeypatch.delenv("T4R_HEAD_AUTO_GB", raising=False)
    cases = [(1024, 100001), (1024, 1000001), (10800, 100001), (256, 10000001), (1, 7)]
    for gb in (None, "0.5", "64"):
        if gb is None:
            monkeypatch.delenv("T4R_HEAD_AUTO_GB", raising=False)
        else:
            monkeypatch.setenv("T4R_HEAD_AUTO_GB", gb)
        for B, V in cases:
            assert P(weight_tying=True).resolve_topk_mode(B, V) == P.size_head_mode(B, V)
            assert P(weight_tying=True, topk_mode="fused").resolve_topk_mode(B, V) == "fused"
            assert P(weight_tying=True, topk_mode="materialize").resolve_topk_mode(B, V) == "materialize"
    monkeypatch.delenv("T4R_HEAD_AUTO_GB", raising=False)
    assert task.resolve_topk_mode(1024, 100001) == "materialize"               # 410 MB: today's path
    assert task.resolve_topk_mode(1024, 10000001) == "fused"                   # 40 GB
    monkeypatch.setenv("T4R_HEAD_AUTO_GB", "0.25")
    assert task.resolve_topk_mode(1024, 100001) == "fused"


def test_operator_is_registered_and_its_fake_gives_the_output_shapes():
    assert "item_topk" in torch_ops.OPERATORS
    schema = str(torch.ops.t4r_hip.item_topk.default._schema)
    assert re.match(r"t4r_hip::item_topk\(Tensor x, Tensor weight, float alpha, (Sym)?[Ii]nt k\) -> \(Tensor, Tensor\)", schema), schema
    x, W = torch.empty(37, 16, device="meta"), torch.empty(1001, 16, device="meta")
    v, i = torch.ops.t4r_hip.item_topk(x, W, 0.5, 20)
    assert v.shape == (37, 20) and v.dtype == torch.float32 and i.shape == (37, 20) and i.dtype == torch.int64
    with FakeTensorMode():
        a, b = torch.empty(5, 16, device="cuda"), torch.empty(300, 16, device="cuda")
        v, i = torch.ops.t4r_hip.item_topk(a, b, 1.0, 7)
        assert v.shape == (5, 7) and i.dtype == torch.int64 and v.device.type == "cuda"


def test_documents_name_the_new_surface():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n = len(_lib.header_symbols())
    with open(os.path.join(root, "README.md")) as f:
        readme = f.read()
    assert re.search(rf"\b{n} entry points", readme), n
    with open(os.path.join(root, "INTEGRATION.md")) as f:
        assert "topk_mode" in f.read()
