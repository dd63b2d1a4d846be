"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/gru_body_clm_train.npz and gru_body_2layer_clm_train.npz: the UNMODIFIED
reference (imported through oracle/ref_standins.py, CPU fp32) on the session model of its tutorial
(examples/tutorial/03-Session-based-recsys.ipynb, section 3.1) and of its unit tests (tests/unit/torch/model/test_head.py), with
the GRU built batch_first so that its time axis is the session:

    SequentialBlock(TabularSequenceFeatures, MLPBlock(dims), Block(torch.nn.GRU(64, 64, num_layers=n, batch_first=True), [None, 20, 64]))

    python tools/make_gru_golden.py

Every fixture: item table 48 wide, L = 20, causal language modeling (no random draw), V = 50 (51 table rows), tied next-item head
(its projection 64 -> 48), B = 8, dropout 0; one training step.  gru_body_clm_train: MLPBlock([64]), one GRU layer;
gru_body_2layer_clm_train: MLPBlock([96, 64]), two GRU layers.
The inputs come from oracle/make_golden.py's synth_inputs (row 0 is a full-length session, row 1 has two items); the parameters
from its reinit.  Keys: p/<state_dict name>, in/<feature>, out/gru_in and out/gru_out (the GRU's input and output tensor, caught by
hooks), out/gru_in_grad and out/gru_out_grad (the gradients that arrive there), out/mask_schema, out/masked_targets, out/loss,
out/predictions, out/labels, g/<parameter name> (the GRU, the MLP stack, the masked-item vector, the item table, the task's
projection), meta/* (with meta/state_dict_keys, the model's state-dict keys joined by newlines): the layout tests/golden_utils.py
reads."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden as mg  # noqa: E402
import ref_standins as rs  # noqa: E402

B, L, V, D_ITEM, D_MODEL = 8, 20, 50, 48, 64
CASES = {"gru_body_clm_train": dict(dimensions=[64], num_layers=1),
         "gru_body_2layer_clm_train": dict(dimensions=[96, 64], num_layers=2)}
BODY = "heads.0.body."
GRADS = (BODY + "1.", BODY + "2.", BODY + "0._masking.", BODY + "0.to_merge.categorical_module.",
         "heads.0.prediction_task_dict.next-item.task_block.")


def build_reference(tr, name):
    """-> the reference Model of fixture `name`"""
    kw = CASES[name]
    schema = mg.make_schema(V, L)
    torch.manual_seed(0)
    feats = tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=L, masking="clm", aggregation="concat",
                                                   embedding_dims={"item_id": D_ITEM})
    gru = torch.nn.GRU(input_size=D_MODEL, hidden_size=D_MODEL, num_layers=kw["num_layers"], batch_first=True)
    body = tr.SequentialBlock(feats, tr.MLPBlock(kw["dimensions"]), tr.Block(gru, [None, L, D_MODEL]))
    model = tr.Model(tr.Head(body, tr.NextItemPredictionTask(weight_tying=True), inputs=feats))
    mg.reinit(model, 1)
    return model


def run(model, x):
    """one training step of the reference -> the fixture's sections"""
    body = model.heads[0].body
    cap = {}

    def pre(m, args):
        a = args[0]
        cap["gru_in"] = a.detach().clone()
        a.register_hook(lambda g: cap.__setitem__("gru_in_grad", g.detach().clone()))

    def post(m, args, out):
        o = out[0]                          # torch.nn.GRU returns (output, h_n)
        cap["gru_out"] = o.detach().clone()
        o.register_hook(lambda g: cap.__setitem__("gru_out_grad", g.detach().clone()))

    gru = body[2].module
    hooks = [gru.register_forward_pre_hook(pre), gru.register_forward_hook(post)]
    model.zero_grad(set_to_none=True)
    try:
        out = model({k: v.clone() for k, v in x.items()}, training=True)
    finally:
        for h in hooks:
            h.remove()
    d = {"in/" + k: v.numpy() for k, v in x.items()}
    seen = set()
    for k, v in model.state_dict().items():
        if v.data_ptr() in seen:            # the same tensor under several names: keep the first
            continue
        seen.add(v.data_ptr())
        d["p/" + k] = v.detach().numpy().copy()
    masking = body[0].masking
    d["out/mask_schema"] = masking.mask_schema.numpy()
    d["out/masked_targets"] = masking.masked_targets.numpy()
    d["out/predictions"] = out["predictions"].detach().numpy()
    d["out/labels"] = out["labels"].numpy()
    d["out/loss"] = out["loss"].detach().numpy()
    out["loss"].backward()
    for k, v in cap.items():
        d["out/" + k] = v.numpy()
    for k, p in model.named_parameters():
        if p.grad is not None and k.startswith(GRADS):
            d["g/" + k] = p.grad.numpy().copy()
    return d


def main():
    tr = rs.import_reference()
    torch.set_num_threads(4)
    x = mg.synth_inputs(B, L, V, (), (), seed=43)
    for name, kw in CASES.items():
        model = build_reference(tr, name)
        model.train()
        d = run(model, x)
        mg.save(name, d, L=L, V=V + 1, d_model=D_MODEL, d_item=D_ITEM, dimensions=",".join(map(str, kw["dimensions"])),
                num_layers=kw["num_layers"], state_dict_keys="\n".join(model.state_dict().keys()))
        print(name, sorted(k for k in d if k.startswith("g/")))


if __name__ == "__main__":
    main()
