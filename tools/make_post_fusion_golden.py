"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/post_fusion_mul_train.npz, post_fusion_sum_train.npz and
post_fusion_concat_train.npz: the UNMODIFIED reference (imported through oracle/ref_standins.py, CPU fp32) on a session model
whose body is transformers4rec/torch/experimental.py's PostContextFusion, built as the reference's own test builds it
(tests/unit/torch/test_experimental.py): SequentialBlock(TabularSequenceFeatures, TransformerBlock) fused with a
SequenceEmbeddingFeatures(aggregation="concat") over one categorical column that does not enter the sequence model.

    python tools/make_post_fusion_golden.py

Every fixture: XLNet d_model 64, 2 layers, 4 heads, L = 20, causal language modeling (no random draw), item table 64 wide, V = 50
(51 table rows), tied next-item head, context column `category` (12 ids + padding, 24 wide), B = 8, dropout 0; one training step.
The inputs come from oracle/make_golden.py's synth_inputs (row 0 is a full-length session, row 1 has two items); the
parameters from its reinit.  To stay below the size limit of a committed file the gradients are stored for the parameters the
tests compare: the context projection, the context table, the masked-item vector, the item table, the task's projection and the
LAST transformer layer.
Keys: p/<state_dict name>, in/<feature>, out/hidden (the transformer block's output), out/context, out/fused (the fusion's
output), out/mask_schema, out/masked_targets, out/loss, out/predictions, out/labels, g/<parameter name>, meta/*: the layout
tests/golden_utils.py reads."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden as mg  # noqa: E402
import ref_standins as rs  # noqa: E402

B, L, V, D_MODEL, N_HEAD, N_LAYER, CAT_CARD, CAT_DIM = 8, 20, 50, 64, 4, 2, 12, 24
CASES = {"post_fusion_mul_train": "elementwise-mul", "post_fusion_sum_train": "elementwise-sum", "post_fusion_concat_train": "concat"}
BODY = "heads.0.body."
GRADS = (BODY + "context_projection.", BODY + "post_context_module.", BODY + "sequential_module.0._masking.",
         BODY + "sequential_module.0.to_merge.categorical_module.", BODY + f"sequential_module.1.transformer.layer.{N_LAYER - 1}.",
         "heads.0.prediction_task_dict.next-item.task_block.")


def build_reference(tr, name):
    """-> the reference Model of fixture `name` (also what tests/test_post_fusion_cpu.py compares state-dict keys with)"""
    from transformers4rec.torch.experimental import PostContextFusion

    schema = mg.make_schema(V, L, cats=(("category", CAT_CARD),))
    torch.manual_seed(0)
    feats = tr.TabularSequenceFeatures.from_schema(schema.select_by_name("item_id"), max_sequence_length=L, masking="clm",
                                                   aggregation="concat", embedding_dims={"item_id": D_MODEL})
    cfg = tr.XLNetConfig.build(d_model=D_MODEL, n_head=N_HEAD, n_layer=N_LAYER, total_seq_length=L, dropout=0.0)
    body = tr.SequentialBlock(feats, tr.TransformerBlock(cfg, masking=feats.masking))
    context = tr.SequenceEmbeddingFeatures.from_schema(schema.select_by_name("category"), aggregation="concat",
                                                       embedding_dims={"category": CAT_DIM})
    fusion = PostContextFusion(body, context, fusion_aggregation=CASES[name])
    model = tr.Model(tr.Head(fusion, tr.NextItemPredictionTask(weight_tying=True), inputs=feats))
    mg.reinit(model, 1)
    return model


def run(model, x):
    """one training step of the reference -> the fixture's sections"""
    fusion = model.heads[0].body
    cap = {}
    hooks = [fusion.sequential_module[1].register_forward_hook(lambda m, i, o: cap.__setitem__("hidden", o.detach().clone())),
             fusion.post_context_module.register_forward_hook(lambda m, i, o: cap.__setitem__(      # the hook sees the features before the concat
                 "context", torch.cat([o[k] for k in sorted(o)], dim=-1).detach().clone() if isinstance(o, dict) else o.detach().clone())),
             fusion.register_forward_hook(lambda m, i, o: cap.__setitem__("fused", o.detach().clone()))]
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
    masking = fusion.sequential_module[0].masking
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
    x = mg.synth_inputs(B, L, V, (("category", CAT_CARD),), (), seed=41)
    for name, aggregation in CASES.items():
        model = build_reference(tr, name)
        model.train()
        d = run(model, x)
        mg.save(name, d, L=L, V=V + 1, d_model=D_MODEL, n_head=N_HEAD, n_layer=N_LAYER, d_item=D_MODEL, cat_card=CAT_CARD,
                cat_dim=CAT_DIM, fusion_aggregation=aggregation)
        print(name, sorted(k for k in d if k.startswith("g/")))


if __name__ == "__main__":
    main()
