"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/xlnet_mlm_contproj_train.npz and xlnet_mlm_contproj2_train.npz: one training
step each of the UNMODIFIED reference (imported through oracle/ref_standins.py, CPU fp32) on a session model whose continuous
columns go through `continuous_projection` (features/tabular.py:90-117, features/sequence.py:271-284).

    python tools/make_contproj_golden.py

B = 8, L = 10, V = 50 (51 table rows), one XLNet layer (d_model 32, 2 heads), dropout 0, MLM.  Three continuous columns named so
that sorting reorders them (the schema lists them as "price", "age_days", "hour"; the first layer's weight columns follow
"age_days", "hour", "price").
  xlnet_mlm_contproj_train   item table 16 wide, one categorical (8 wide), continuous_projection=24, concat, d_output 32
  xlnet_mlm_contproj2_train  item table and categorical 16 wide, continuous_projection=[12, 16], element-wise-sum (every width
                             16), d_output 32
Conventions of the .npz as in oracle/make_golden.py."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden as mg  # noqa: E402
import ref_standins as rs  # noqa: E402

B, L, V, D_MODEL, N_HEAD = 8, 10, 50, 32, 2
CATS = (("category", 7),)
CONTS = ("price", "age_days", "hour")
CASES = {
    "xlnet_mlm_contproj_train": dict(dims=24, aggregation="concat", d_item=16, d_cat=8),
    "xlnet_mlm_contproj2_train": dict(dims=[12, 16], aggregation="element-wise-sum", d_item=16, d_cat=16),
}


def build_reference(tr, name):
    """-> the reference Model of fixture `name` (also what tests/test_cont_proj_cpu.py compares state-dict keys with)"""
    c = CASES[name]
    schema = mg.make_schema(V, L, CATS, CONTS)
    torch.manual_seed(0)
    kw = dict(max_sequence_length=L, embedding_dims={"item_id": c["d_item"], "category": c["d_cat"]}, continuous_projection=c["dims"])
    if c["aggregation"] == "concat":
        feats = tr.TabularSequenceFeatures.from_schema(schema, masking="mlm", aggregation="concat", d_output=D_MODEL, **kw)
    else:
        # the reference's from_schema sizes the block BEFORE it projects the continuous columns, so an element-wise aggregation
        # fails there on the width-1 raw columns: aggregate, project and mask afterwards, with the calls from_schema itself makes
        from transformers4rec.torch.block.mlp import MLPBlock
        from transformers4rec.torch.masking import masking_registry

        feats = tr.TabularSequenceFeatures.from_schema(schema, **kw)
        feats.aggregation = c["aggregation"]
        feats.projection_module = MLPBlock([D_MODEL]).build(feats.output_size())
        feats.set_masking(masking_registry.parse("mlm")(hidden_size=feats.output_size()[-1]))
    cfg = tr.XLNetConfig.build(d_model=D_MODEL, n_head=N_HEAD, n_layer=1, total_seq_length=L, dropout=0.0)
    model = cfg.to_torch_model(feats, tr.NextItemPredictionTask(weight_tying=True))
    mg.reinit(model, 1)
    return model


def main():
    tr = rs.import_reference()
    torch.set_num_threads(4)
    for i, (name, c) in enumerate(CASES.items()):
        model = build_reference(tr, name)
        x = mg.synth_inputs(B, L, V, CATS, CONTS, seed=21 + i)
        model.train()
        d = mg.run(model, x, training=True, testing=False, want_grads=True)
        dims = [c["dims"]] if isinstance(c["dims"], int) else c["dims"]
        mg.save(name, d, L=L, V=V + 1, d_model=D_MODEL, n_head=N_HEAD, n_layer=1, d_item=c["d_item"], d_cat=c["d_cat"],
                dims=dims, aggregation=c["aggregation"])
        for k in d:
            if k.startswith(("p/", "g/")) and "continuous_module" in k:
                print(k, d[k].shape)


if __name__ == "__main__":
    main()
