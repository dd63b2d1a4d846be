"""Host half of the half-precision serving head (csrc/item_topk_h16.hip): the C ABI carries the entries, argument errors
come back as messages, the workspace stays far below the score matrix, the operators are registered with fakes, the task
validates prepare_serving, host tensors are refused.  Nothing here needs a GPU."""
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import transformers4rec_amd as tr
from transformers4rec_amd import _lib, ops, torch_ops

ENTRIES = ("t4r_item_table_image_ld", "t4r_item_table_pack_h16", "t4r_item_scores_h16", "t4r_item_topk_h16_ws_bytes",
           "t4r_item_topk_h16")


def test_library_exports_and_header_declares_the_entry_points():
    lib = _lib.load()
    syms = _lib.header_symbols()
    for name in ENTRIES + ("t4r_item_topk_h16_supported",):
        assert name in syms and hasattr(lib, name) and name in _lib.signatures(), name
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    decl = text[: text.index("t4r_item_table_image_ld(int")]
    comment = decl[decl.rindex("/*"):]
    for cite in ("prediction_task.py:664", ":452-470", "trainer.py:363-367"):         # the reference lines it replaces
        assert cite in comment, cite


def test_image_pitch_and_supported_widths():
    lib = _lib.load()
    for D in (1, 7, 8, 16, 17, 48, 100, 128, 255, 256, 500, 512, 513, 1000):
        ld = lib.t4r_item_table_image_ld(D)
        assert ld % 8 == 0 and D <= ld < D + 16, (D, ld)
        assert ops.image_ld(D) == ld
    assert lib.t4r_item_table_image_ld(0) == 0
    assert [lib.t4r_item_topk_h16_supported(D) for D in (0, 1, 512, 513)] == [0, 1, 1, 0]
    assert ops.item_topk_h16_supported(512) and not ops.item_topk_h16_supported(513)


def test_workspace_is_far_below_the_score_matrix():
    lib = _lib.load()
    for N, V, D, k in [(1024, 100001, 128, 20), (1024, 1000001, 256, 100), (256, 10000001, 512, 10)]:
        ws = lib.t4r_item_topk_h16_ws_bytes(N, V, D, k)
        assert 0 < ws < 4 * N * ops.pad_ld(V) / 8, (N, V, D, k, ws)
    assert lib.t4r_item_topk_h16_ws_bytes(1, 7, 8, 7) > 0
    assert lib.t4r_item_topk_h16_ws_bytes(0, 7, 8, 7) == 0


def test_workspace_sizes_are_the_recorded_ones():
    """(N, V, D, k) -> bytes, as the build before the two heads got one driver returned them: the plan did not move"""
    ws = _lib.load().t4r_item_topk_h16_ws_bytes
    for shape, b in [((1, 7, 8, 7), 1536), ((12, 5000, 32, 10), 248320), ((37, 4099, 100, 1), 767488),
                     ((1024, 100001, 128, 20), 33808640), ((1024, 1000001, 256, 100), 233496832),
                     ((256, 10000001, 512, 10), 71031808)]:
        assert ws(*shape) == b, (shape, ws(*shape), b)


def test_argument_errors_come_back_as_messages():
    lib = _lib.load()
    rc = lib.t4r_item_topk_h16(None, 4, 100, 8, 1.0, None, 8, None, 16, 3, 10, None, None, None, 0, None)
    assert rc != 0 and b"item_topk_h16" in lib.t4r_last_error()
    rc = lib.t4r_item_scores_h16(None, 4, 100, 8, 1.0, None, 8, None, 16, 3, None, 128, None, 0)
    assert rc != 0 and b"item_scores_h16" in lib.t4r_last_error()
    rc = lib.t4r_item_table_pack_h16(None, None, 8, 100, 8, 3, None, 16)
    assert rc != 0 and b"item_table_pack_h16" in lib.t4r_last_error()
    # a dtype code that is no 16-bit format, a width beyond the supported ones: refused before anything is touched
    rc = lib.t4r_item_table_pack_h16(None, 64, 8, 100, 8, 0, 64, 16)
    assert rc != 0 and b"dtype" in lib.t4r_last_error()
    rc = lib.t4r_item_topk_h16(None, 4, 100, 600, 1.0, 64, 600, 64, 608, 3, 10, 64, 64, 64, 1 << 30, None)
    assert rc != 0 and b"512" in lib.t4r_last_error()
    # zero rows: nothing to do
    assert lib.t4r_item_topk_h16(None, 0, 100, 8, 1.0, None, 8, None, 16, 3, 10, None, None, None, 0, None) == 0


def test_host_tensors_are_refused():
    x, W = torch.randn(4, 8), torch.randn(50, 8)
    with pytest.raises(_lib.T4RHipError):
        ops.pack_item_table(W, "fp16")
    with pytest.raises(_lib.T4RHipError):
        torch.ops.t4r_hip.pack_item_table(W, "bf16")
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(_lib.T4RHipError):           # host tensors raise first, whatever the dtype
            ops.item_topk(x, W.to(dt), 5)
        with pytest.raises(_lib.T4RHipError):
            ops.item_scores(x, W.to(dt))
        with pytest.raises(_lib.T4RHipError):
            torch.ops.t4r_hip.item_topk(x, W.to(dt), 1.0, 5)
    with pytest.raises(ValueError):
        ops.pack_item_table(W, "fp8")
    st = ops.item_topk_stats()
    assert {"calls", "calls_h16", "dtype", "fallback_rows"} <= set(st)


def test_operators_are_registered_and_their_fakes_give_the_output_shapes():
    assert "pack_item_table" in torch_ops.OPERATORS
    schema = str(torch.ops.t4r_hip.pack_item_table.default._schema)
    assert re.match(r"t4r_hip::pack_item_table\(Tensor weight, str dtype\) -> Tensor", schema), schema
    # schemas of the two consumers are what they were
    assert re.match(r"t4r_hip::item_topk\(Tensor x, Tensor weight, float alpha, (Sym)?[Ii]nt k\) -> \(Tensor, Tensor\)",
                    str(torch.ops.t4r_hip.item_topk.default._schema))
    assert re.match(r"t4r_hip::item_scores\(Tensor x, Tensor weight, float alpha\) -> Tensor",
                    str(torch.ops.t4r_hip.item_scores.default._schema))
    for name, td in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        W = torch.empty(1001, 100, device="meta")
        img = torch.ops.t4r_hip.pack_item_table(W, name)
        assert img.shape == (1001, 100) and img.dtype == td and img.stride() == (ops.image_ld(100), 1)
        x = torch.empty(37, 100, device="meta")
        v, i = torch.ops.t4r_hip.item_topk(x, img, 0.5, 20)
        assert v.shape == (37, 20) and v.dtype == torch.float32 and i.shape == (37, 20) and i.dtype == torch.int64
        s = torch.ops.t4r_hip.item_scores(x, img, 0.5)
        assert s.shape == (37, 1001) and s.dtype == torch.float32
        with FakeTensorMode():
            a, b = torch.empty(5, 16, device="cuda"), torch.empty(300, 16, device="cuda")
            im = torch.ops.t4r_hip.pack_item_table(b, name)
            assert im.shape == (300, 16) and im.dtype == td and im.device.type == "cuda"
            v, i = torch.ops.t4r_hip.item_topk(a, im, 1.0, 7)
            assert v.shape == (5, 7) and v.dtype == torch.float32 and i.dtype == torch.int64 and v.device.type == "cuda"
            s = torch.ops.t4r_hip.item_scores(a, im, 1.0)
            assert s.shape == (5, 300) and s.dtype == torch.float32 and s.stride(0) % 64 == 0
    with pytest.raises(Exception):
        torch.ops.t4r_hip.pack_item_table(torch.empty(10, 8, device="meta"), "fp8")


def test_prepare_serving_validation():
    task = tr.NextItemPredictionTask(weight_tying=True)
    assert task.serving_dtype is None and task.serving_packs == 0
    with pytest.raises(ValueError):
        task.prepare_serving("fp32")
    with pytest.raises(ValueError):
        task.prepare_serving("int8")
    with pytest.raises(RuntimeError):                   # not built yet: no weights to pack
        task.prepare_serving("fp16")
    task.drop_serving_image()                           # harmless without an image
    assert task.serving_dtype is None
    # the image is no parameter and no buffer: checkpoints do not change
    L, V, D = 20, 500, 32
    schema = tr.session_schema(V - 1, L)
    inputs = tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=L, masking="mlm", embedding_dim_default=D)
    model = tr.XLNetConfig.build(D, 4, 1, total_seq_length=L, dropout=0.0).to_torch_model(
        inputs, tr.NextItemPredictionTask(weight_tying=True))
    keys = list(model.state_dict().keys())
    with pytest.raises(_lib.T4RHipError):               # host weights: refused by the pack, and nothing is left half set
        model.prediction_task.prepare_serving("bf16")
    assert list(model.state_dict().keys()) == keys
