"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/mlp_body_clm_train.npz and mlp_body_linear_clm_train.npz: the UNMODIFIED
reference (imported through oracle/ref_standins.py, CPU fp32) on a session model whose body is the one its README, its
docs/source/model_definition.md and most of its unit tests build:

    SequentialBlock(TabularSequenceFeatures, MLPBlock(dims), TransformerBlock)

    python tools/make_mlp_block_golden.py

Every fixture: item table 48 wide (the input block's width, so also the masked-item vector's), XLNet d_model 64, 2 layers, 4 heads,
L = 20, causal language modeling (no random draw), V = 50 (51 table rows), tied next-item head (its projection 64 -> 48), B = 8,
dropout 0; one training step.  mlp_body_clm_train: MLPBlock([96, 64]) (Linear + ReLU twice); mlp_body_linear_clm_train:
MLPBlock([64], activation=None, use_bias=False).
The inputs come from oracle/make_golden.py's synth_inputs (row 0 is a full-length session, row 1 has two items); the
parameters from its reinit.  To stay below the size limit of a committed file the gradients are stored for the parameters the
tests compare: the stack, the masked-item vector, the item table, the task's projection and the LAST transformer layer.
Keys: p/<state_dict name>, in/<feature>, out/mlp (the stack's output), out/hidden (the transformer block's output),
out/mask_schema, out/masked_targets, out/loss, out/predictions, out/labels, g/<parameter name>, meta/*: the layout
tests/golden_utils.py reads."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden as mg  # noqa: E402
import ref_standins as rs  # noqa: E402

B, L, V, D_ITEM, D_MODEL, N_HEAD, N_LAYER = 8, 20, 50, 48, 64, 4, 2
CASES = {"mlp_body_clm_train": dict(dimensions=[96, 64]),
         "mlp_body_linear_clm_train": dict(dimensions=[64], activation=None, use_bias=False)}
BODY = "heads.0.body."
GRADS = (BODY + "1.", BODY + "0._masking.", BODY + "0.to_merge.categorical_module.", BODY + f"2.transformer.layer.{N_LAYER - 1}.",
         "heads.0.prediction_task_dict.next-item.task_block.")


def build_reference(tr, name):
    """-> the reference Model of fixture `name` (also what tests/test_mlp_block_cpu.py compares state-dict keys with)"""
    schema = mg.make_schema(V, L)
    torch.manual_seed(0)
    feats = tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=L, masking="clm", aggregation="concat",
                                                   embedding_dims={"item_id": D_ITEM})
    cfg = tr.XLNetConfig.build(d_model=D_MODEL, n_head=N_HEAD, n_layer=N_LAYER, total_seq_length=L, dropout=0.0)
    body = tr.SequentialBlock(feats, tr.MLPBlock(**CASES[name]), tr.TransformerBlock(cfg, masking=feats.masking))
    model = tr.Model(tr.Head(body, tr.NextItemPredictionTask(weight_tying=True), inputs=feats))
    mg.reinit(model, 1)
    return model


def run(model, x):
    """one training step of the reference -> the fixture's sections"""
    body = model.heads[0].body
    cap = {}
    hooks = [body[1].register_forward_hook(lambda m, i, o: cap.__setitem__("mlp", o.detach().clone())),
             body[2].register_forward_hook(lambda m, i, o: cap.__setitem__("hidden", o.detach().clone()))]
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
    for k, v in cap.items():
        d["out/" + k] = v.numpy()
    d["out/predictions"] = out["predictions"].detach().numpy()
    d["out/labels"] = out["labels"].numpy()
    d["out/loss"] = out["loss"].detach().numpy()
    out["loss"].backward()
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
        mg.save(name, d, L=L, V=V + 1, d_model=D_MODEL, n_head=N_HEAD, n_layer=N_LAYER, d_item=D_ITEM,
                dimensions=",".join(map(str, kw["dimensions"])), relu=int(kw.get("activation", True) is not None),
                use_bias=int(kw.get("use_bias", True)))
        print(name, sorted(k for k in d if k.startswith("g/")))


if __name__ == "__main__":
    main()
