"""Host half of the session-level tasks: the eleventh C-ABI header (include/t4r_hip_seqtask.h) against its ctypes table, the size
query and the argument limits (refused before any launch), the registered operators' fakes, the float64 restatement
(tests/session_task_restatement.py) against the reference's own tasks built live (oracle/ref_standins.py) and against the
committed fixtures (tools/make_session_task_golden.py), names and state-dict keys, the refusals, the Head / Model output
contracts, last_rows_gate and the documents.  Nothing here needs a GPU."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch

import golden_utils as gu
import session_task_restatement as R
import transformers4rec_amd as tr
from transformers4rec_amd import _lib, model as model_mod, ops, session_task as st, torch_ops  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOUR = ["t4r_seq_task_bwd", "t4r_seq_task_fwd", "t4r_seq_task_supported", "t4r_seq_task_ws_floats"]
CLICK, DWELL = "click/binary_classification_task", "dwell/regression_task"
TD = "heads.0.prediction_task_dict."


# ---------------------------------------------------------------------------------------------------------- header and ABI
def test_seqtask_header_library_and_prototypes_agree():
    lib = _lib.load()
    syms = _lib.header_symbols("t4r_hip_seqtask.h")
    assert syms == FOUR
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/t4r_hip_seqtask.h but not exported"
    text = open(_lib.header_path("t4r_hip_seqtask.h")).read()
    for entry in ("int t4r_seq_task_fwd(void* stream", "int t4r_seq_task_bwd(void* stream"):
        decl = text[: text.index(entry)]
        comment = decl[decl.rindex("/*"):]
        assert "replaces:" in comment and "model/prediction_task.py:66-303" in comment, entry
    decls = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for word in ("at::", "torch", "Tensor", "std::", "c10"):
        assert word not in decls, f"{word} leaked into the C ABI"


def test_ws_floats_is_pure_and_monotone():
    f = _lib.load().t4r_seq_task_ws_floats
    assert f(0, 64) == 0 and f(-3, 64) == 0 and f(8, 0) == 0 and f(8, 1025) == 0
    Bs = [1, 3, 31, 32, 33, 65, 1024, 8191, 8192, 8193, 100000, 3_000_000]
    for D in (1, 6, 64, 130, 1024):
        got = [f(B, D) for B in Bs]
        assert got == [f(B, D) for B in Bs] and got == sorted(got) and got[0] >= 1 + D + 1, (D, got)
    for B in (1, 65, 100000):
        got = [f(B, D) for D in (1, 4, 6, 64, 100, 130, 1024)]
        assert got == sorted(got) and got[0] > 0, got


BUF = ctypes.c_void_p(1 << 20)        # never dereferenced: every failing case below is refused before any launch


def _fwd(lib, L=3, D=8, summary=0, act=1, loss_kind=1, B=4, x=BUF):
    return lib.t4r_seq_task_fwd(None, x, None, B, L, D, summary, BUF, None, act, loss_kind, BUF, BUF, BUF, BUF, BUF)


def _bwd(lib, L=3, D=8, summary=0, act=1, loss_kind=1, B=4, dx=BUF):
    return lib.t4r_seq_task_bwd(None, BUF, BUF, BUF, BUF, None, B, L, D, summary, BUF, act, loss_kind, dx, None, None, BUF)


def test_limits_and_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    assert [lib.t4r_seq_task_supported(*a) for a in ((1, 1), (1023, 1024), (0, 8), (1024, 8), (3, 0), (3, 1025))] == [1, 1, 0, 0, 0, 0]
    for call in (_fwd, _bwd):
        for kw, word in ((dict(L=0), b"L"), (dict(L=1024), b"L"), (dict(D=0), b"D"), (dict(D=1025), b"D"),
                         (dict(summary=3), b"summary"), (dict(summary=-1), b"summary"), (dict(act=2), b"act"),
                         (dict(loss_kind=2), b"loss_kind"), (dict(act=0, loss_kind=1), b"BCE"), (dict(B=-1), b"B")):
            assert call(lib, **kw) < 0, (call.__name__, kw)
            assert word in lib.t4r_last_error(), (call.__name__, kw, lib.t4r_last_error())
    assert _fwd(lib, x=None) < 0 and b"null" in lib.t4r_last_error()
    assert _bwd(lib, dx=None) < 0 and b"null" in lib.t4r_last_error()
    assert lib.t4r_seq_task_fwd(None, ctypes.c_void_p((1 << 20) + 2), None, 4, 3, 8, 0, BUF, None, 1, 1, BUF, BUF, BUF, BUF, BUF) < 0
    assert b"aligned" in lib.t4r_last_error()
    # B = 0: nothing launches, nothing is looked at
    assert lib.t4r_seq_task_fwd(None, None, None, 0, 3, 8, 0, None, None, 1, 1, None, None, None, None, None) == 0
    assert lib.t4r_seq_task_bwd(None, None, None, None, None, None, 0, 3, 8, 0, None, 1, 1, None, None, None, None) == 0
    x, w = torch.zeros(2, 3, 8), torch.zeros(8)
    with pytest.raises(_lib.T4RHipError, match="GPU"):
        ops.seq_task_fwd(x, None, w, None, torch.zeros(2), 0, 1, 1)
    with pytest.raises(_lib.T4RHipError, match="GPU"):
        ops.seq_task_bwd_(torch.ones(1), torch.zeros(2), torch.zeros(2), torch.zeros(2, 8), None, 3, w, 0, 1, 1)


def test_operators_are_registered_and_their_fakes_give_the_shapes():
    assert {"seq_task_fwd", "seq_task_bwd"} <= set(torch_ops.OPERATORS)
    for name in ("seq_task_fwd", "seq_task_bwd"):
        assert str(getattr(torch.ops.t4r_hip, name).default._schema).startswith(f"t4r_hip::{name}(")
    m = lambda *s, **k: torch.empty(*s, device="meta", **k)     # noqa: E731
    s, pred, loss = torch.ops.t4r_hip.seq_task_fwd(m(5, 7, 6), m(5, dtype=torch.int32), m(6), m(1), m(5), 2, 0, 0)
    assert (s.shape, pred.shape, loss.shape) == ((5, 6), (5,), (1,))
    s, pred, loss = torch.ops.t4r_hip.seq_task_fwd(m(5, 7, 6), None, m(1, 6), None, None, 0, 1, 1)
    assert (s.shape, pred.shape, loss.shape) == ((5, 6), (5,), (0,))
    dx, dw, db = torch.ops.t4r_hip.seq_task_bwd(m(1), m(5), m(5), m(5, 6), None, 7, m(1, 6), True, 2, 0, 0)
    assert (dx.shape, dw.shape, db.shape) == ((5, 7, 6), (1, 6), (1,))
    assert torch.ops.t4r_hip.seq_task_bwd(m(1), m(5), m(5), m(5, 6), None, 7, m(6), False, 2, 1, 1)[2].shape == (0,)


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_restatement_counts_clamps_and_empty_sessions():
    x = torch.arange(2 * 3 * 2, dtype=torch.float64).reshape(2, 3, 2) + 1
    lens = torch.tensor([0, 7])
    assert R.counts(2, 3, lens).tolist() == [0, 3] and R.counts(2, 3).tolist() == [3, 3]
    for mode in (R.FIRST, R.LAST, R.MEAN):
        s = R.summary_of(x, mode, lens)
        assert torch.equal(s[0], torch.zeros(2, dtype=torch.float64))
        assert torch.equal(R.coef(2, 3, mode, lens)[0], torch.zeros(3, dtype=torch.float64))
    assert torch.equal(R.summary_of(x, R.LAST, torch.tensor([2, 3])), torch.stack([x[0, 1], x[1, 2]]))
    assert torch.equal(R.summary_of(x, R.MEAN, torch.tensor([2, 3]))[0], (x[0, 0] + x[0, 1]) / 2)
    # the -100 clamp of both logarithms and the 1e-12 clamp of the BCE gradient
    p, t = torch.tensor([0.0, 1.0, 1.0, 0.0, 0.25]), torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0])
    rows = R.row_losses(p, t, R.BCE)
    assert rows[:4].tolist() == [100.0, 100.0, 0.0, 0.0] and abs(float(rows[4]) - 1.3862943611198906) < 1e-12
    dz = R.dz_of(p, t, 1.0, 1, R.BCE)
    assert dz[:4].tolist() == [0.0, 0.0, 0.0, 0.0] and abs(float(dz[4]) - (0.25 - 1.0) / 5) < 1e-15
    tiny = torch.tensor([1e-14], dtype=torch.float64)
    assert abs(float(R.dz_of(tiny, torch.tensor([1.0]), 1.0, 1, R.BCE)) - (1e-14 - 1) * 1e-14 * (1 - 1e-14) / 1e-12) < 1e-16
    assert torch.equal(R.dz_of(p, t, 2.0, 0, R.MSE), 2.0 / 5 * 2 * (p - t).double())


# ------------------------------------------------------------------------------------------------ against the reference, live
def _tool():
    spec = importlib.util.spec_from_file_location("make_session_task_golden", os.path.join(ROOT, "tools", "make_session_task_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _reference():
    import ref_standins as rs

    if not os.path.isdir(rs.REFERENCE_ROOT):
        pytest.skip("the reference tree is not on this machine")
    return rs.import_reference(), _tool()


def _close64(got, want, what):
    scale = max(float(want.abs().max()), 1e-300)
    assert float((got.double() - want.double()).abs().max()) <= 1e-12 * scale, what


@pytest.mark.parametrize("summary", ["first", "last", "mean"])
@pytest.mark.parametrize("kind", ["binary", "regression"])
def test_restatement_equals_the_reference_tasks_in_float64(summary, kind):
    ref_tr, _mod = _reference()
    B, L, D = 5, 4, 6
    g = torch.Generator().manual_seed(7)
    cls = ref_tr.BinaryClassificationTask if kind == "binary" else ref_tr.RegressionTask
    task = cls("y", summary_type=summary)
    task.build(None, (-1, L, D))
    task = task.double()
    hidden = torch.randn(B, L, D, generator=g, dtype=torch.float64).requires_grad_(True)
    target = torch.randint(0, 2, (B,), generator=g).double() if kind == "binary" else torch.randn(B, generator=g, dtype=torch.float64)
    out = task(hidden, targets=target, training=True)
    (3.0 * out["loss"]).backward()
    lin = task.pre[0]
    act, loss_kind = (1, R.BCE) if kind == "binary" else (0, R.MSE)
    mode = ops.SUMMARY[summary]
    r = R.forward(hidden.detach(), lin.weight.detach(), lin.bias.detach() if lin.bias is not None else None, target, mode, act, loss_kind)
    dz = R.dz_of(r["pred"], target, 3.0, act, loss_kind)
    dx, dw, db = R.backward(dz, r["s"], lin.weight.detach(), L, mode)
    _close64(r["loss"], out["loss"].detach(), "loss")
    _close64(r["pred"], out["predictions"].detach(), "predictions")
    _close64(dx, hidden.grad, "d hidden")
    _close64(dw, lin.weight.grad.reshape(-1), "d weight")
    if lin.bias is not None:
        _close64(db.reshape(1), lin.bias.grad, "d bias")
    else:
        assert kind == "binary"


def test_names_target_dim_and_state_dict_keys_equal_the_reference():
    ref_tr, mod = _reference()
    for name in ("session_tasks_train", "session_tasks_multi_train"):
        ref = mod.build_reference(ref_tr, name)
        ours = _mirror(name)
        ref_tasks, our_tasks = ref.heads[0].prediction_task_dict, ours.heads[0].prediction_task_dict
        assert list(ref_tasks.keys()) == list(our_tasks.keys())
        for k in ref_tasks:
            assert ref_tasks[k].task_name == our_tasks[k].task_name == k
            if k != "next-item":
                assert ref_tasks[k].target_dim == our_tasks[k].target_dim == 1
        sr = {k: tuple(v.shape) for k, v in ref.state_dict().items() if k.startswith(TD) and "next-item" not in k}
        so = {k: tuple(v.shape) for k, v in ours.state_dict().items() if k.startswith(TD) and "next-item" not in k}
        assert sr == so == {TD + CLICK + ".pre.0.weight": (1, 64), TD + DWELL + ".pre.0.weight": (1, 64), TD + DWELL + ".pre.0.bias": (1,)}
    for cls, rcls in ((tr.BinaryClassificationTask, ref_tr.BinaryClassificationTask), (tr.RegressionTask, ref_tr.RegressionTask)):
        assert cls().task_name == rcls().task_name and cls("t").task_name == rcls("t").task_name
        assert cls("t", task_name="mine").task_name == rcls("t", task_name="mine").task_name == "mine"


# ------------------------------------------------------------------------------------------------ fixtures
SPEC = {"session_tasks_train": ((CLICK, "click", "mean", 1, R.BCE), (DWELL, "dwell", "last", 0, R.MSE)),
        "session_tasks_multi_train": ((CLICK, "click", "first", 1, R.BCE), (DWELL, "dwell", "mean", 0, R.MSE))}


@pytest.mark.parametrize("name", ["session_tasks_train", "session_tasks_infer", "session_tasks_multi_train"])
def test_restatement_equals_the_fixtures_from_their_stored_hidden(name):
    d = gu.load(name)
    assert os.path.getsize(os.path.join(gu.GOLDEN, name + ".npz")) < (1 << 20)
    hidden = gu.t(d["out/hidden"])
    assert hidden.shape == (8, 6, 64) and (gu.t(d["in/item_id"])[1] != 0).sum() == 2 and (gu.t(d["in/item_id"])[0] != 0).all()
    total = []
    for task, target, summary, act, loss_kind in SPEC["session_tasks_train" if name == "session_tasks_infer" else name]:
        w = gu.t(d[f"p/{TD}{task}.pre.0.weight"])
        b = gu.t(d[f"p/{TD}{task}.pre.0.bias"]) if f"p/{TD}{task}.pre.0.bias" in d else None
        tg = gu.t(d["in/targets/" + target]) if name != "session_tasks_infer" else None
        r = R.forward(hidden, w, b, tg, ops.SUMMARY[summary], act, loss_kind)
        torch.testing.assert_close(r["pred"].float(), gu.t(d["out/predictions/" + task]), rtol=1e-5, atol=1e-6)
        if tg is None:
            continue
        torch.testing.assert_close(r["loss"].float(), gu.t(d["out/loss/" + task]), rtol=1e-5, atol=1e-6)
        assert torch.equal(gu.t(d["out/labels/" + task]), tg)
        total.append(r["loss"])
        # the parameter gradients of the task: the step's loss weighs it by w_i / (number of tasks)
        n_tasks = 2 if name == "session_tasks_train" else 3
        wt = dict(zip((CLICK, DWELL), d["meta/task_weights"].tolist()))[task] if name == "session_tasks_train" else 1.0
        dz = R.dz_of(r["pred"], tg, wt / n_tasks, act, loss_kind)
        _dx, dw, db = R.backward(dz, r["s"], w, 6, ops.SUMMARY[summary])
        torch.testing.assert_close(dw.float().reshape(1, -1), gu.t(d[f"g/{TD}{task}.pre.0.weight"]), rtol=1e-4, atol=1e-6)
        if b is not None:
            torch.testing.assert_close(db.float().reshape(1), gu.t(d[f"g/{TD}{task}.pre.0.bias"]), rtol=1e-4, atol=1e-6)
    if name == "session_tasks_train":
        w1, w2 = d["meta/task_weights"].tolist()
        torch.testing.assert_close(((w1 * total[0] + w2 * total[1]) / 2).float(), gu.t(d["out/loss"]), rtol=1e-5, atol=1e-6)
        # the second batch differs in row 2 only, whose last position is padding
        a, b2 = gu.t(d["in/item_id"]), gu.t(d["in2/item_id"])
        assert (a != b2).nonzero().tolist() == [[2, 5]] and int(b2[2, 5]) == 0
    if name == "session_tasks_multi_train":
        ni = gu.t(d["out/loss/next-item"]).double()
        torch.testing.assert_close(((ni + total[0] + total[1]) / 3).float(), gu.t(d["out/loss"]), rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------ construction and refusals
def _mirror(name, **task_kw):
    mod = _tool()
    c = mod.CASES["session_tasks_train" if name == "session_tasks_infer" else name]
    feats = tr.TabularSequenceFeatures.from_schema(tr.session_schema(mod.V, mod.L), max_sequence_length=mod.L, masking=c["masking"],
                                                   aggregation="concat", embedding_dims={"item_id": mod.D_MODEL})
    cfg = tr.XLNetConfig.build(d_model=mod.D_MODEL, n_head=mod.N_HEAD, n_layer=1, total_seq_length=mod.L, dropout=0.0)
    tasks = []
    for t in c["tasks"]:
        if t[0] == "next-item":
            tasks.append(tr.NextItemPredictionTask(weight_tying=True))
        else:
            tasks.append((tr.BinaryClassificationTask if t[0] == "binary" else tr.RegressionTask)(t[1], summary_type=t[2], **task_kw))
    return cfg.to_torch_model(feats, *tasks, task_weights=c["task_weights"])


def test_construction_defaults_and_parameters():
    t = tr.BinaryClassificationTask("click")
    assert (t.summary_type, t.mask_padding, t.target_dim, t.target_name) == ("first", False, 1, "click")
    assert isinstance(t.loss, torch.nn.BCELoss) and [type(m) for m in t.metrics] == [st.Precision, st.Recall, st.Accuracy]
    r = tr.RegressionTask("dwell", summary_type="cls_index")
    assert isinstance(r.loss, torch.nn.MSELoss) and [type(m) for m in r.metrics] == [st.MeanSquaredError] and r._summary == ops.SUMMARY["last"]
    torch.manual_seed(0)
    t.build(body=None, input_size=(-1, 6, 64))
    r.build(body=None, input_size=(-1, 6, 64), inputs=None, device=None, task_block=None, pre=None)
    assert {k: tuple(v.shape) for k, v in t.state_dict().items()} == {"pre.0.weight": (1, 64)}
    assert {k: tuple(v.shape) for k, v in r.state_dict().items()} == {"pre.0.weight": (1, 64), "pre.0.bias": (1,)}
    assert 0 < float(t.pre[0].weight.detach().abs().max()) <= 1 / 8      # torch.nn.Linear's init: U(-1/sqrt(D), 1/sqrt(D))
    assert [t.metric_name(m) for m in t.metrics] == [CLICK + "/precision", CLICK + "/recall", CLICK + "/accuracy"]
    assert [r.metric_name(m) for m in r.metrics] == [DWELL + "/mean_squared_error"]
    model = _mirror("session_tasks_train")
    carried = {id(p) for p in tr.hip_parameters(model)}
    named = dict(model.named_parameters())
    for k in (TD + CLICK + ".pre.0.weight", TD + DWELL + ".pre.0.weight", TD + DWELL + ".pre.0.bias"):
        assert id(named[k]) in carried, k
    dense, _tables = tr.flatten_model(model)
    flat = {n for n, *_ in dense.entries}
    assert {TD + CLICK + ".pre.0.weight", TD + DWELL + ".pre.0.bias"} <= flat


def test_refusals():
    for cls in (tr.BinaryClassificationTask, tr.RegressionTask):
        with pytest.raises(NotImplementedError, match="task_block"):
            cls("y", task_block=torch.nn.Linear(4, 4))
        with pytest.raises(NotImplementedError, match="attn"):
            cls("y", summary_type="attn")
        with pytest.raises(NotImplementedError, match="summary_type=None"):
            cls("y", summary_type=None)
        with pytest.raises(ValueError, match="summary_type"):
            cls("y", summary_type="median")
        with pytest.raises(NotImplementedError, match="loss"):
            cls("y", loss=torch.nn.L1Loss())
        with pytest.raises(NotImplementedError, match="task_block"):
            cls("y").build(body=None, input_size=(-1, 6, 64), task_block=torch.nn.Linear(4, 4))
        with pytest.raises(ValueError, match="3-dim"):
            cls("y").build(body=None, input_size=(-1, 64))
    with pytest.raises(NotImplementedError, match="loss"):
        tr.BinaryClassificationTask("y", loss=torch.nn.MSELoss())
    with pytest.raises(NotImplementedError, match="loss"):
        tr.BinaryClassificationTask("y", loss=torch.nn.BCELoss(reduction="sum"))
    with pytest.raises(NotImplementedError, match="loss"):
        tr.BinaryClassificationTask("y", loss=torch.nn.BCELoss(weight=torch.ones(3)))
    with pytest.raises(NotImplementedError, match="loss"):
        tr.RegressionTask("y", loss=torch.nn.MSELoss(reduction="none"))
    t = tr.BinaryClassificationTask("y", summary_type="mean", mask_padding=True).build(body=None, input_size=(-1, 6, 8))
    with pytest.raises(ValueError, match="inputs"):
        t(torch.zeros(2, 6, 8), targets=torch.zeros(2), training=True)
    with pytest.raises(RuntimeError, match="not built"):
        tr.RegressionTask("y")(torch.zeros(2, 6, 8))
    with pytest.raises(ValueError, match="named"):
        tr.Head(None, [tr.RegressionTask("y"), tr.RegressionTask("y")])


# ------------------------------------------------------------------------------------------------ Head / Model contracts
class _StubTask(torch.nn.Module):
    """a session task without a kernel: what Head / Model do with the tasks' outputs can be checked on the CPU"""

    def __init__(self, target_name, value):
        super().__init__()
        self.target_name, self.task_name, self.value, self.seen = target_name, target_name + "/stub", value, None

    def build(self, **kw):
        return self

    def forward(self, h, targets=None, training=False, testing=False):
        self.seen = targets
        pred = torch.full((h.shape[0],), self.value)
        if training or testing:
            return {"loss": torch.tensor(self.value), "labels": targets, "predictions": pred}
        return pred


class _StubBody(torch.nn.Module):
    def forward(self, inputs, training=False, testing=False, **kw):
        assert "out_rows" not in kw or kw["out_rows"] is None
        return torch.zeros(inputs["item_id"].shape[0], 3, 4)


def _stub_model(tasks, **kw):
    m = tr.Model.__new__(tr.Model)
    torch.nn.Module.__init__(m)
    m.heads = torch.nn.ModuleList([tr.Head(_StubBody(), tasks, **kw)])
    m.max_sequence_length, m.top_k, m.exclude_seen = None, None, False
    return m


def test_head_and_model_output_contracts():
    a, b = _StubTask("click", 2.0), _StubTask("dwell", 4.0)
    m = _stub_model([a, b], task_weights=[1.0, 0.5])
    assert list(m.heads[0].prediction_task_dict.keys()) == ["click/stub", "dwell/stub"]
    x = {"item_id": torch.ones(5, 3, dtype=torch.int64)}
    tg = {"click": torch.ones(5, dtype=torch.int64), "dwell": torch.arange(5)}
    out = m(x, targets=tg, training=True)
    assert float(out["loss"]) == (2.0 * 1.0 + 4.0 * 0.5) / 2
    assert set(out["labels"]) == set(out["predictions"]) == {"click/stub", "dwell/stub"}
    assert a.seen.dtype == torch.float32 and torch.equal(b.seen, torch.arange(5).float())      # cast to float, picked by target_name
    assert float(_stub_model([a, b], loss_reduction="sum")(x, targets=tg, testing=True)["loss"]) == 6.0
    m(x, targets=torch.zeros(5), training=True)
    assert torch.equal(a.seen, torch.zeros(5)) and torch.equal(b.seen, torch.zeros(5))          # one tensor goes to every task
    inf = m(x)
    assert set(inf) == {"click/stub", "dwell/stub"} and inf["dwell/stub"].shape == (5,)
    # one task: the dicts collapse to the bare values (the reference's len(labels) == 1 rule)
    one = _stub_model(a)
    out = one(x, targets=tg, training=True)
    assert torch.is_tensor(out["labels"]) and torch.is_tensor(out["predictions"]) and float(out["loss"]) == 2.0
    assert torch.is_tensor(one(x)) and one(x).shape == (5,)
    assert one.prediction_task is a and one.prediction_tasks == [a] and m.prediction_tasks == [a, b]


def test_metrics_follow_the_reference_definitions():
    t = tr.BinaryClassificationTask("click").build(body=None, input_size=(-1, 3, 4))
    p, y = torch.tensor([0.9, 0.8, 0.2, 0.6, 0.4]), torch.tensor([1.0, 0.0, 0.0, 1.0, 1.0])
    got = t.calculate_metrics(p, y)
    assert {k: round(float(v), 6) for k, v in got.items()} == {CLICK + "/precision": round(2 / 3, 6), CLICK + "/recall": round(2 / 3, 6),
                                                               CLICK + "/accuracy": 0.6}
    t.calculate_metrics(torch.tensor([0.1]), torch.tensor([1.0]))
    acc = t.compute_metrics()
    assert abs(float(acc[CLICK + "/recall"]) - 0.5) < 1e-6 and abs(float(acc[CLICK + "/accuracy"]) - 0.5) < 1e-6
    t.reset_metrics()
    assert float(t.compute_metrics()[CLICK + "/accuracy"]) == 0.0
    r = tr.RegressionTask("dwell").build(body=None, input_size=(-1, 3, 4))
    assert abs(float(r.calculate_metrics(torch.tensor([1.0, 3.0]), torch.tensor([0.0, 1.0]))[DWELL + "/mean_squared_error"]) - 2.5) < 1e-6
    m = _mirror("session_tasks_train")
    m.calculate_metrics({CLICK: p, DWELL: p}, {CLICK: y, DWELL: y})
    assert set(m.compute_metrics()) == {CLICK + "/precision", CLICK + "/recall", CLICK + "/accuracy", DWELL + "/mean_squared_error"}
    m.reset_metrics()


def test_last_rows_gate_is_closed_for_session_tasks():
    from transformers4rec_amd import transformer as tfm

    multi = _mirror("session_tasks_multi_train")
    multi.train()
    lone_session = tr.XLNetConfig.build(d_model=64, n_head=2, n_layer=1, total_seq_length=6, dropout=0.0).to_torch_model(
        tr.TabularSequenceFeatures.from_schema(tr.session_schema(50, 6), max_sequence_length=6, masking="clm", aggregation="concat",
                                               embedding_dims={"item_id": 64}), tr.BinaryClassificationTask("click"))
    lone_session.train()
    assert isinstance(multi.prediction_task, tr.NextItemPredictionTask)       # the gate used to look at this one only
    assert model_mod.last_rows_gate(multi, True, 64, 6, n_labels=8) is None
    assert model_mod.last_rows_gate(lone_session, True, 64, 6, n_labels=8) is None
    # a lone next-item model: the answer depends on the library's shape queries only, exactly as before
    feats = tr.TabularSequenceFeatures.from_schema(tr.session_schema(50, 6), max_sequence_length=6, masking="clm", aggregation="concat",
                                                   embedding_dims={"item_id": 64})
    lone = tr.XLNetConfig.build(d_model=64, n_head=2, n_layer=1, total_seq_length=6, dropout=0.0).to_torch_model(
        feats, tr.NextItemPredictionTask(weight_tying=True))
    lone.train()
    want = 8 if (tfm._LAST_ROWS and tfm._FUSED_ON and ops.xlnet_fused_supported(64) and ops.xlnet_attn_block_supported(6, 64, 2)
                 and 8 <= tfm._LAST_ROWS_MAX_FRACTION * 64 * 6) else None
    assert model_mod.last_rows_gate(lone, True, 64, 6, n_labels=8) == want
    assert lone._single_next_item() and not multi._single_next_item() and not lone_session._single_next_item()


# ---------------------------------------------------------------------------------------------------------- documents
def test_documents_name_the_new_surface():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "125 entry points" in readme                                                     # the pinned phrases stay
    assert "the 4 session-task entry points of `include/t4r_hip_seqtask.h`" in readme
    assert readme.count("t4r_hip_seqtask.h") >= 2 and "seq_task.hip" in readme              # the first paragraph and the layout list
    for word in ("BinaryClassificationTask", "RegressionTask", "session_task.py"):
        assert word in readme, word
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for word in FOUR + ["t4r_hip_seqtask.h", "BinaryClassificationTask", "RegressionTask", "mask_padding", "task_weights", "loss_reduction",
                        "pre.0.weight", "Head.from_schema", "convert_model", "task_block"]:
        assert word in integ, word
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 4.11" in design and "seq_task.hip" in design
    assert "seq_task.hip" in open(os.path.join(ROOT, "transformers4rec_amd", "build.py")).read()
    for tool in ("seq_task_bench.py", "make_session_task_golden.py"):
        assert os.path.exists(os.path.join(ROOT, "tools", tool))
    header = open(_lib.header_path("t4r_hip_seqtask.h")).read()
    for phrase in ("no float atomics", "EVERY element is written", "ACCUMULATED", "B = 0: nothing launches"):
        assert phrase in header, phrase
