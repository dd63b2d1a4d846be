"""Host half of the one-pass evaluation head over the serving image (csrc/item_eval_h16.hip): the C ABI carries the two
entries, the workspace size is a pure function, argument errors come back as messages before any launch, the operator is
registered with a fake, host tensors and an fp32 table are refused, an unbuilt task raises.  Nothing here needs a GPU."""
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import transformers4rec_amd as tr
from transformers4rec_amd import _lib, ops, torch_ops

ENTRIES = ("t4r_item_eval_h16_ws_bytes", "t4r_item_eval_h16")


def test_library_exports_and_header_declares_the_entry_points():
    lib = _lib.load()
    syms = _lib.header_symbols()
    for name in ENTRIES:
        assert name in syms and hasattr(lib, name) and name in _lib.signatures(), name
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    decl = text[: text.index("t4r_item_eval_h16_ws_bytes(int")]
    comment = decl[decl.rindex("/*"):]
    for cite in ("trainer.py:363-367", "prediction_task.py:430", "ranking_metric.py:52-59"):   # the reference chain it replaces
        assert cite in comment, cite


def test_workspace_size_is_pure_positive_and_monotone():
    ws = _lib.load().t4r_item_eval_h16_ws_bytes
    for D in (1, 20, 128, 512):
        prev_n = 0
        for N in (1, 2, 37, 128, 129, 1024, 4096):
            b = ws(N, 100001, D)
            assert b > 0 and b >= prev_n and b == ws(N, 100001, D), (N, D, b)
            prev_n = b
        prev_v = 0
        for V in (1, 63, 64, 65, 1001, 100001, 131072, 131073, 1000001, 10000001, 20000000, 100000000):
            b = ws(300, V, D)
            assert b > 0 and b >= prev_v and b == ws(300, V, D), (V, D, b)
            prev_v = b
    for N, V, D in [(0, 100, 8), (-1, 100, 8), (4, 0, 8), (4, -5, 8), (4, 100, 0), (4, 100, -1)]:
        assert ws(N, V, D) == 0, (N, V, D)
    # far below the score matrix at the three serving shapes
    for N, V, D in [(1024, 100001, 128), (1024, 1000001, 256), (256, 10000001, 512)]:
        assert ws(N, V, D) < 4 * N * ops.pad_ld(V) / 8, (N, V, D, ws(N, V, D))


def test_workspace_sizes_are_the_recorded_ones():
    """(N, V, D) -> bytes, as the build before the image contract moved into item_h16_tile.h returned them (the shapes of the
    two top-k heads' tables, without their k)"""
    ws = _lib.load().t4r_item_eval_h16_ws_bytes
    for shape, b in [((1, 7, 8), 272), ((12, 5000, 32), 15936), ((37, 4099, 100), 46928), ((1024, 100001, 128), 25870336),
                     ((1024, 1000001, 256), 34078720), ((256, 10000001, 512), 10264576)]:
        assert ws(*shape) == b, (shape, ws(*shape), b)


def test_argument_errors_come_back_as_messages_before_any_launch():
    lib = _lib.load()
    P, WS = 64, 1 << 30           # never dereferenced: every call below is refused by the argument checks

    def call(n=4, V=100, D=8, ldx=8, ldp=16, dtype=3, labels=P, x=P, image=P, outs=(P, P, P, P), ws=P, ws_bytes=WS):
        return lib.t4r_item_eval_h16(None, n, V, D, 1.0, x, ldx, image, ldp, dtype, labels, *outs, ws, ws_bytes)

    assert call(D=513, ldx=513, ldp=528) != 0 and b"512" in lib.t4r_last_error()
    assert call(dtype=1) != 0 and b"dtype" in lib.t4r_last_error()
    assert call(dtype=0) != 0 and b"dtype" in lib.t4r_last_error()
    assert call(labels=None) != 0 and b"item_eval_h16" in lib.t4r_last_error() and b"labels" in lib.t4r_last_error()
    assert call(x=None) != 0 and b"item_eval_h16" in lib.t4r_last_error()
    assert call(outs=(P, None, P, P)) != 0 and b"item_eval_h16" in lib.t4r_last_error()
    assert call(ldx=7) != 0 and b"pitch" in lib.t4r_last_error()
    assert call(ldp=8) != 0 and b"image" in lib.t4r_last_error()
    assert call(image=72) != 0 and b"image" in lib.t4r_last_error()              # not 16-byte aligned
    assert call(ws_bytes=16) != 0 and b"workspace" in lib.t4r_last_error()
    assert call(ws=None) != 0 and b"workspace" in lib.t4r_last_error()
    assert call(V=0) != 0 and call(n=-1) != 0
    assert call(n=0, labels=None, x=None) == 0                                   # zero rows: nothing to do


def test_operator_is_registered_and_its_fake_gives_the_four_outputs():
    assert "item_eval" in torch_ops.OPERATORS
    schema = str(torch.ops.t4r_hip.item_eval.default._schema)
    assert re.match(r"t4r_hip::item_eval\(Tensor x, Tensor weight, Tensor labels, float alpha\) -> "
                    r"\(Tensor, Tensor, Tensor, Tensor\)", schema), schema

    def check(out, n, dev):
        assert len(out) == 4
        for t, dt in zip(out, (torch.float32, torch.float32, torch.float32, torch.int32)):
            assert t.shape == (n,) and t.dtype == dt and t.device.type == dev

    for td in (torch.float16, torch.bfloat16):
        x = torch.empty(37, 100, device="meta")
        img = torch.empty(1001, 112, device="meta", dtype=td)[:, :100]
        y = torch.empty(37, device="meta", dtype=torch.int64)
        check(torch.ops.t4r_hip.item_eval(x, img, y, 0.5), 37, "meta")
        with FakeTensorMode():
            a = torch.empty(5, 16, device="cuda")
            im = torch.empty(300, 16, device="cuda", dtype=td)
            lab = torch.empty(5, device="cuda", dtype=torch.int64)
            check(torch.ops.t4r_hip.item_eval(a, im, lab, 1.0), 5, "cuda")


def test_host_tensors_and_an_fp32_table_are_refused():
    x, W, y = torch.randn(4, 8), torch.randn(50, 8), torch.tensor([1, 2, 3, 4])
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(_lib.T4RHipError, match="no CPU path"):
            ops.item_eval(x, W.to(dt), y)
        with pytest.raises(_lib.T4RHipError, match="no CPU path"):
            torch.ops.t4r_hip.item_eval(x, W.to(dt), y, 1.0)
    with pytest.raises(TypeError, match="pack_item_table"):       # an fp32 table is the caller's likeliest mistake: say what to do
        ops.item_eval(x, W, y)
    with pytest.raises(TypeError, match="pack_item_table"):
        torch.ops.t4r_hip.item_eval(x, W, y, 1.0)


def test_evaluate_batch_on_an_unbuilt_task_raises():
    task = tr.NextItemPredictionTask(weight_tying=True)
    with pytest.raises(RuntimeError, match="not built"):
        task.evaluate_batch(torch.zeros(2, 3, 8))
