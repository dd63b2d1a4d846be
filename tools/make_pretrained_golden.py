"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/xlnet_mlm_pretrained_train.npz: one training step of the UNMODIFIED reference
(imported through oracle/ref_standins.py, CPU fp32) on a session model whose input block merges a pretrained-embedding module
(PretrainedEmbeddingFeatures, torch/features/embedding.py:599-740) next to the item table.

    python tools/make_pretrained_golden.py

B = 8, L = 10, V = 50 (51 table rows), item table 16 wide; one pretrained feature `item_vec`, E = 40 projected to 24 with
"layer-norm"; concat, d_output 32, one XLNet layer (d_model 32, 2 heads), dropout 0.  The pretrained inputs are
table.half().float()[item_ids]: what a device-resident fp16 image of the table holds exactly.  Conventions of the .npz as in
oracle/make_golden.py, plus `table/item_vec` (the fp32 table the inputs were looked up in).  The reference modules are
constructed directly (its from_schema needs the merlin schema's shape properties, which the stand-ins do not model)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden as mg  # noqa: E402
import ref_standins as rs  # noqa: E402

NAME = "xlnet_mlm_pretrained_train"
B, L, V, D_ITEM, E, P, D_MODEL, N_HEAD = 8, 10, 50, 16, 40, 24, 32, 2
FEATURE = "item_vec"


def build_reference(tr):
    """-> the reference Model (also what tests/test_pretrained_cpu.py compares state-dict keys with)"""
    from transformers4rec.torch.block.mlp import MLPBlock
    from transformers4rec.torch.features.embedding import PretrainedEmbeddingFeatures
    from transformers4rec.torch.masking import masking_registry

    schema = mg.make_schema(V, L)
    torch.manual_seed(0)
    base = tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=L, aggregation="concat",
                                                  embedding_dim_default=D_ITEM, pretrained_embeddings_tags=None)
    pre = PretrainedEmbeddingFeatures([FEATURE], pretrained_output_dims=P, normalizer="layer-norm")
    feats = tr.TabularSequenceFeatures(categorical_module=base.to_merge["categorical_module"], pretrained_embedding_module=pre,
                                       aggregation="concat", schema=schema)
    feats.build({"item_id": torch.Size([-1, L]), FEATURE: torch.Size([-1, L, E])}, schema=schema)
    hidden = feats.output_size()
    feats.projection_module = MLPBlock([D_MODEL]).build(hidden)
    feats.set_masking(masking_registry.parse("mlm")(hidden_size=feats.output_size()[-1]))
    cfg = tr.XLNetConfig.build(d_model=D_MODEL, n_head=N_HEAD, n_layer=1, total_seq_length=L, dropout=0.0)
    model = cfg.to_torch_model(feats, tr.NextItemPredictionTask(weight_tying=True))
    mg.reinit(model, 1)
    return model


def main():
    tr = rs.import_reference()
    torch.set_num_threads(4)
    model = build_reference(tr)
    x = mg.synth_inputs(B, L, V, (), (), seed=11)
    g = torch.Generator().manual_seed(12)
    table = torch.randn((V + 1, E), generator=g)
    x[FEATURE] = table.half().float()[x["item_id"]]
    model.train()
    d = mg.run(model, x, training=True, testing=False, want_grads=True)
    d["table/" + FEATURE] = table.numpy()
    mg.save(NAME, d, L=L, V=V + 1, d_model=D_MODEL, n_head=N_HEAD, n_layer=1, E=E, P=P, d_item=D_ITEM)
    for k in d:
        if k.startswith(("p/", "g/")) and ("pretrained" in k or "projection_module" in k):
            print(k, d[k].shape)


if __name__ == "__main__":
    main()
