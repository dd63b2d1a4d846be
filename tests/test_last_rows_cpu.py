"""CPU checks of the row-mapped last layer: the seventh header against the library and the derived prototypes, and the Python gate
(model.last_rows_gate) that decides whether a training step may run the last XLNet layer on the label rows only."""
import torch

import transformers4rec_amd as tr
from transformers4rec_amd import _lib, model as model_mod, transformer as tfm


def test_rows_header_is_exported_and_bound():
    lib = _lib.load()
    syms = _lib.header_symbols("t4r_hip_rows.h")
    assert syms == ["t4r_xlnet_ff_bwd_rows", "t4r_xlnet_ff_fwd_rows", "t4r_xlnet_layer_bwd_rows", "t4r_xlnet_layer_fwd_rows",
                    "t4r_xlnet_ln1_bwd_rows"]
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/t4r_hip_rows.h but not exported"
    # every mapped entry = its plain entry + the map (rows, n) at the end: tests/test_abi_headers_cpu.py
    hdr = open(_lib.header_path("t4r_hip_rows.h")).read()
    for word in ("at::", "torch", "Tensor", "std::", "c10"):
        assert word not in hdr


def test_rows_entries_refuse_bad_arguments_without_a_gpu():
    """checked before any launch: no device is touched, so this runs anywhere"""
    lib = _lib.load()
    one = 8       # any non-null address: the checks below fail before it is looked at
    for name, lead in (("t4r_xlnet_layer_fwd_rows", (None,) * 6), ("t4r_xlnet_layer_bwd_rows", (None,) * 9)):
        fn = getattr(lib, name)
        tail = (0.03, 0.0, 0, 0, 0)
        assert fn(*lead, 2, 20, 64, 4, *tail, None, None, one, 0) != 0 and b"mapped rows" in lib.t4r_last_error()
        assert fn(*lead, 2, 20, 64, 4, *tail, None, None, one, 41) != 0 and b"mapped rows" in lib.t4r_last_error()
        assert fn(*lead, 2, 20, 48, 4, *tail, None, None, one, 5) != 0 and b"token-tile" in lib.t4r_last_error()
        assert fn(*lead, 2, 40, 64, 4, *tail, None, None, one, 5) != 0 and b"one-kernel attention" in lib.t4r_last_error()
        assert fn(*lead, 2, 20, 64, 4, *tail, one, None, one, 5) != 0 and b"key_len" in lib.t4r_last_error()
        assert fn(*lead, 2, 20, 64, 4, *tail, None, None, None, 5) != 0 and b"null row map" in lib.t4r_last_error()


def _model(D=64, masking="mlm", weight_tying=True, mask_padding=False, task=None):
    L = 20
    schema = tr.session_schema(999, L)
    inputs = tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=L, masking=masking, embedding_dim_default=D)
    cfg = tr.XLNetConfig.build(D, 4, 2, total_seq_length=L, dropout=0.3)
    block = tr.TransformerBlock(cfg, masking=inputs.masking, mask_padding=mask_padding)
    return model_mod.Model(inputs, block, task or tr.NextItemPredictionTask(weight_tying=weight_tying)).train()


def test_gate_engages_only_where_nothing_reads_the_other_rows(monkeypatch):
    B, L = 64, 20
    gate = model_mod.last_rows_gate
    m = _model()
    assert gate(m, True, B, L, n_labels=190) == 190
    assert gate(m, True, B, L, n_labels=B * L // 2) == B * L // 2
    # the row rule: 2 n <= B L; and never an empty map
    assert gate(m, True, B, L, n_labels=B * L // 2 + 1) is None
    assert gate(m, True, B, L, n_labels=0) is None
    # evaluation (testing=True arrives here as training=False), eval mode, no-grad
    assert gate(m, False, B, L, n_labels=190) is None
    with torch.no_grad():
        assert gate(m, True, B, L, n_labels=190) is None
    m.eval()
    assert gate(m, True, B, L, n_labels=190) is None
    m.train()
    # the switch
    monkeypatch.setattr(tfm, "_LAST_ROWS", False)
    assert gate(m, True, B, L, n_labels=190) is None
    monkeypatch.setattr(tfm, "_LAST_ROWS", True)
    # the opt-in padding mask
    assert gate(_model(mask_padding=True), True, B, L, n_labels=190) is None
    # a width / length the fused path refuses
    assert gate(_model(D=48), True, B, L, n_labels=190) is None
    assert gate(m, True, B, 40, n_labels=190) is None
    # a head that is not the tied next-item head itself: it may read more than the label rows
    assert gate(_model(weight_tying=False), True, B, L, n_labels=190) is None

    class Custom(tr.NextItemPredictionTask):
        pass

    assert gate(_model(task=Custom(weight_tying=True)), True, B, L, n_labels=190) is None
    # somebody else reads the body's output
    h = m.transformer_block.register_forward_hook(lambda *a: None)
    assert gate(m, True, B, L, n_labels=190) is None
    h.remove()
    assert gate(m, True, B, L, n_labels=190) == 190


def test_direct_calls_keep_every_row():
    """out_rows is a keyword only Model.forward sets: the signatures default to None"""
    import inspect

    for fn in (tfm.XLNetModel.forward, tfm.TransformerBlock.forward):
        assert inspect.signature(fn).parameters["out_rows"].default is None
    from transformers4rec_amd import ops

    for fn in (ops.xlnet_layer_fwd, ops.xlnet_layer_bwd):
        ps = inspect.signature(fn).parameters
        assert ps["rows"].default is None and ps["n_rows"].default is None
