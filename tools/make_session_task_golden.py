"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/session_tasks_train.npz, session_tasks_infer.npz and
session_tasks_multi_train.npz: the UNMODIFIED reference (imported through oracle/ref_standins.py, CPU fp32) on session models
with the session-level tasks (transformers4rec/torch/model/prediction_task.py:66-303) under a multi-task Head
(model/base.py:235-425).

    python tools/make_session_task_golden.py

Every fixture: one XLNet layer, d_model 64 (2 heads), item table 64 wide, V = 50 (51 table rows), B = 8, L = 6, dropout 0; the
inputs come from oracle/make_golden.py's synth_inputs (row 0 is a full-length session, row 1 has two items).
  session_tasks_train        masking=None; binary "click" (mean) + regression "dwell" (last), task_weights [1.0, 0.5]; one
                             training step with every gradient.  A second batch (in2/, out2/), forward only, differs from the
                             first in row 2, whose last position is emptied (item id 0): what mask_padding changes.
  session_tasks_infer        the same model, inference
  session_tasks_multi_train  causal language modeling (no random draw); NextItemPredictionTask(weight_tying=True) + binary "click"
                             (first) + regression "dwell" (mean); one training step with every gradient
Keys: p/<state_dict name>, in/<feature>, in/targets/<target>, out/hidden, out/loss, out/loss/<task>, out/predictions/<task>,
out/labels/<task>, g/<parameter name>, meta/*: the layout tests/golden_utils.py reads."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden as mg  # noqa: E402
import ref_standins as rs  # noqa: E402

B, L, V, D_MODEL, N_HEAD = 8, 6, 50, 64, 2
CLICK, DWELL = "click/binary_classification_task", "dwell/regression_task"
CASES = {
    "session_tasks_train": dict(masking=None, tasks=(("binary", "click", "mean"), ("regression", "dwell", "last")),
                                task_weights=[1.0, 0.5]),
    "session_tasks_multi_train": dict(masking="clm", tasks=(("next-item",), ("binary", "click", "first"),
                                                            ("regression", "dwell", "mean")), task_weights=None),
}


def build_reference(tr, name):
    """-> the reference Model of fixture `name` (also what tests/test_session_task_cpu.py compares names and keys with)"""
    c = CASES["session_tasks_train" if name == "session_tasks_infer" else name]
    schema = mg.make_schema(V, L)
    torch.manual_seed(0)
    feats = tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=L, masking=c["masking"], aggregation="concat",
                                                   embedding_dims={"item_id": D_MODEL})
    cfg = tr.XLNetConfig.build(d_model=D_MODEL, n_head=N_HEAD, n_layer=1, total_seq_length=L, dropout=0.0)
    body = tr.SequentialBlock(feats, tr.TransformerBlock(cfg, masking=feats.masking))
    tasks = []
    for t in c["tasks"]:
        if t[0] == "next-item":
            tasks.append(tr.NextItemPredictionTask(weight_tying=True))
        else:
            cls = tr.BinaryClassificationTask if t[0] == "binary" else tr.RegressionTask
            tasks.append(cls(t[1], summary_type=t[2]))
    model = tr.Model(tr.Head(body, tasks, task_weights=c["task_weights"], inputs=feats))
    mg.reinit(model, 1)
    return model


def targets(seed):
    g = torch.Generator().manual_seed(seed)
    return {"click": torch.randint(0, 2, (B,), generator=g).float(), "dwell": torch.randn((B,), generator=g)}


def run(model, x, tg, training, want_grads, prefix=("in/", "out/")):
    """one call of the reference -> the fixture's sections"""
    pin, pout = prefix
    cap = {}
    hook = model.heads[0].body[1].register_forward_hook(lambda m, i, o: cap.__setitem__("hidden", o.detach().clone()))
    model.zero_grad(set_to_none=True)
    tasks = model.heads[0].prediction_task_dict
    try:
        if training:
            out = model({k: v.clone() for k, v in x.items()}, targets={k: v.clone() for k, v in tg.items()}, training=True)
        else:
            out = model({k: v.clone() for k, v in x.items()})
    finally:
        hook.remove()
    d = {pin + k: v.numpy() for k, v in x.items()}
    d[pout + "hidden"] = cap["hidden"].numpy()
    if not training:
        out = out if isinstance(out, dict) else {next(iter(tasks)): out}
        for name, v in out.items():
            d[pout + "predictions/" + name] = v.detach().numpy()
        return d
    for k, v in tg.items():
        d[pin + "targets/" + k] = v.numpy()
    d[pout + "loss"] = out["loss"].detach().numpy()
    for name in tasks:
        d[pout + "predictions/" + name] = out["predictions"][name].detach().numpy()
        d[pout + "labels/" + name] = out["labels"][name].detach().numpy()
    # the task losses one at a time, from the same body output (what the step's loss reduces)
    with torch.no_grad():
        for name, task in tasks.items():
            o = task(cap["hidden"], targets=tg.get(task.target_name), training=True)
            d[pout + "loss/" + name] = o["loss"].numpy()
    if want_grads:
        out["loss"].backward()
        for k, p in model.named_parameters():
            if p.grad is not None:
                d["g/" + k] = p.grad.numpy().copy()
    return d


def params(model):
    d, seen = {}, set()
    for k, v in model.state_dict().items():
        if v.data_ptr() in seen:            # the same tensor under several names: keep the first
            continue
        seen.add(v.data_ptr())
        d["p/" + k] = v.detach().numpy().copy()
    return d


def main():
    tr = rs.import_reference()
    torch.set_num_threads(4)
    meta = dict(L=L, V=V + 1, d_model=D_MODEL, n_head=N_HEAD, n_layer=1, d_item=D_MODEL)
    x = mg.synth_inputs(B, L, V, (), (), seed=31)
    x["item_id"][2, :] = torch.randint(1, V + 1, (L,), generator=torch.Generator().manual_seed(5))     # row 2: full length ...
    x2 = {k: v.clone() for k, v in x.items()}
    x2["item_id"][2, L - 1] = 0                                                                         # ... and one item short
    tg = targets(32)

    model = build_reference(tr, "session_tasks_train")
    model.train()
    d = params(model)
    d.update(run(model, x, tg, training=True, want_grads=True))
    d.update(run(model, x2, tg, training=True, want_grads=False, prefix=("in2/", "out2/")))
    mg.save("session_tasks_train", d, task_weights=CASES["session_tasks_train"]["task_weights"], **meta)

    model.eval()
    d = params(model)
    d.update(run(model, x, None, training=False, want_grads=False))
    mg.save("session_tasks_infer", d, **meta)

    model = build_reference(tr, "session_tasks_multi_train")
    model.train()
    d = params(model)
    d.update(run(model, x, tg, training=True, want_grads=True))
    masking = model.heads[0].body[0].masking
    d["out/mask_schema"] = masking.mask_schema.numpy()
    d["out/masked_targets"] = masking.masked_targets.numpy()
    mg.save("session_tasks_multi_train", d, **meta)
    for k in sorted(d):
        if "prediction_task_dict" in k:
            print(k, d[k].shape)


if __name__ == "__main__":
    main()
