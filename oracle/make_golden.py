"""TEST INFRASTRUCTURE ONLY.  Generates tests/golden/*.npz by running the UNMODIFIED
reference (NVIDIA-Merlin/Transformers4Rec at /root/reference, imported through
oracle/ref_standins.py) on CPU fp32 with fixed seeds.

    python oracle/make_golden.py            # (re)writes tests/golden/*.npz
    python oracle/make_golden.py --long     # only the long-sequence fixtures (round 6)

The fixtures pin the oracle (oracle/t4r_oracle.py) and, through it and directly, the HIP
path.  /root/reference is absent on the GPU box, so only the .npz files travel.

Conventions inside each .npz
  in/<feature>            model inputs  [B,L]
  p/<state_dict key>      every parameter/buffer of the reference model (state_dict names;
                          aliases of one tensor stored once; *_eval/*_infer cases reuse the
                          parameters of the matching *_train file)
  draw/bern, draw/j1, draw/j2, draw/neg   recorded torch.bernoulli / torch.multinomial draws
  draw/ssn_bern/<module>/<feature>, draw/ssn_perm/<module>/<feature>   StochasticSwapNoise draws
  draw/post_keep/<feature>                TabularDropout keep masks of the categorical module
  out/mask_schema, out/masked_targets, out/inputs_embeds, out/hidden,
  out/predictions, out/labels, out/loss
  g/<state_dict key>      d loss / d param   (training cases)
  meta/*                  scalars (n_head, d_model, eps, ...)
Weights are re-drawn N(0, 0.1) (biases N(0,0.1), LN weight 1+N(0,0.1)) so that indexing
mistakes are visible far above fp32 rounding; dropout=0.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_standins as rs  # noqa: E402
from ref_standins import ColumnSchema, Schema, Tags, _IntDomain, _ValueCount  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")
SHARD_BYTES = 900 * 1024          # compressed bytes per fixture file (the repository keeps every file under 1 MiB)


class DrawRecorder:
    """Records torch.bernoulli / torch.multinomial results while the reference runs."""

    def __init__(self):
        self.bern, self.multi = [], []

    def __enter__(self):
        self._b, self._m = torch.bernoulli, torch.multinomial

        def bern(*a, **k):
            r = self._b(*a, **k)
            self.bern.append(r.clone())
            return r

        def multi(*a, **k):
            r = self._m(*a, **k)
            self.multi.append(r.clone())
            return r

        torch.bernoulli, torch.multinomial = bern, multi
        return self

    def __exit__(self, *exc):
        torch.bernoulli, torch.multinomial = self._b, self._m


def make_schema(V, L, cats=(), conts=()):
    cols = [ColumnSchema("item_id", tags=[Tags.CATEGORICAL, Tags.ITEM_ID, Tags.LIST, Tags.ITEM],
                         int_domain=_IntDomain(0, V), value_count=_ValueCount(1, L))]
    for name, card in cats:
        cols.append(ColumnSchema(name, tags=[Tags.CATEGORICAL, Tags.LIST],
                                 int_domain=_IntDomain(0, card), value_count=_ValueCount(1, L)))
    for name in conts:
        cols.append(ColumnSchema(name, tags=[Tags.CONTINUOUS, Tags.LIST],
                                 value_count=_ValueCount(1, L)))
    return Schema(cols)


def synth_inputs(B, L, V, cats, conts, seed, min_len=1):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(min_len, L + 1, (B,), generator=g)
    lens[0] = L  # a full-length session
    lens[1] = max(min_len, 2)
    m = torch.arange(L)[None] < lens[:, None]
    x = {"item_id": torch.randint(1, V + 1, (B, L), generator=g) * m}
    for name, card in cats:
        x[name] = torch.randint(1, card + 1, (B, L), generator=g) * m
    for name in conts:
        x[name] = torch.rand((B, L), generator=g) * m
    return x


def reinit(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "layer_norm" in n and n.endswith("weight"):
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))


def build(tr, V, L, d_model, n_head, n_layer, cats=(), conts=(), masking="mlm",
          aggregation="concat", d_output=None, embedding_dims=None, emb_default=None,
          weight_tying=True, sampled_softmax=False, max_n_samples=100, seed=0, arch="xlnet"):
    schema = make_schema(V, L, cats, conts)
    kw = dict(max_sequence_length=L, masking=masking, aggregation=aggregation)
    if d_output:
        kw["d_output"] = d_output
    if conts:
        kw["continuous_soft_embeddings"] = True
    if embedding_dims:
        kw["embedding_dims"] = embedding_dims
    if emb_default:
        kw["embedding_dim_default"] = emb_default
    torch.manual_seed(seed)
    inputs = tr.TabularSequenceFeatures.from_schema(schema, **kw)
    if arch == "xlnet":
        cfg = tr.XLNetConfig.build(d_model=d_model, n_head=n_head, n_layer=n_layer,
                                   total_seq_length=L, dropout=0.0)
    elif arch == "gpt2":
        cfg = tr.GPT2Config.build(d_model=d_model, n_head=n_head, n_layer=n_layer,
                                  total_seq_length=L, dropout=0.0)
    else:  # BertConfig.build ignores its `dropout` argument (HF defaults 0.1 stay): zero them explicitly
        from transformers4rec.config import transformer as tconf

        cfg = tconf.BertConfig.build(d_model=d_model, n_head=n_head, n_layer=n_layer, total_seq_length=L,
                                  hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    task = tr.NextItemPredictionTask(weight_tying=weight_tying, sampled_softmax=sampled_softmax,
                                     max_n_samples=max_n_samples)
    model = cfg.to_torch_model(inputs, task)
    reinit(model, seed + 1)
    return model


def run(model, x, training, testing, want_grads, with_params=True):
    cap = {}
    body = model.heads[0].body
    h0 = body[0].register_forward_hook(lambda m, i, o: cap.__setitem__("inputs_embeds", o.detach().clone()))
    h1 = body[1].register_forward_hook(lambda m, i, o: cap.__setitem__("hidden", o.detach().clone()))
    model.zero_grad(set_to_none=True)
    with DrawRecorder() as rec:
        out = model({k: v.clone() for k, v in x.items()}, training=training, testing=testing)
    h0.remove()
    h1.remove()
    d = {}
    for k, v in x.items():
        d["in/" + k] = v.numpy()
    seen = set()
    for k, v in model.state_dict().items():
        # the same tensor is registered under several names; keep the first
        if not with_params or v.data_ptr() in seen:
            continue
        seen.add(v.data_ptr())
        d["p/" + k] = v.detach().numpy().copy()
    masking = body[0].masking
    d["out/mask_schema"] = masking.mask_schema.numpy()
    d["out/masked_targets"] = masking.masked_targets.numpy()
    d["out/inputs_embeds"] = cap["inputs_embeds"].numpy()
    d["out/hidden"] = cap["hidden"].numpy()
    if isinstance(out, dict):
        d["out/predictions"] = out["predictions"].detach().numpy()
        d["out/labels"] = out["labels"].numpy()
        d["out/loss"] = out["loss"].detach().numpy()
        if want_grads:
            out["loss"].backward()
            sd_params = dict(model.named_parameters())
            for k, p in sd_params.items():
                if p.grad is not None:
                    d["g/" + k] = p.grad.numpy().copy()
    else:
        d["out/predictions"] = out.detach().numpy()
    if rec.bern:
        d["draw/bern"] = rec.bern[-1].numpy()   # the MLM draw is the last one (swap-noise draws precede it)
    mlm = masking.__class__.__name__ == "MaskedLanguageModeling"
    multi = list(rec.multi)
    if mlm and training:
        d["draw/j1"] = multi[0].reshape(-1).numpy()
        d["draw/j2"] = multi[1].reshape(-1).numpy()
        multi = multi[2:]
    if multi:  # sampled softmax: the sampler's multinomial (2n tries)
        d["draw/neg_tries"] = multi[0].numpy()
    return d


def save(name, d, **meta):
    for k, v in meta.items():
        d["meta/" + k] = np.asarray(v)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **d)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB, loss={d.get('out/loss')}")
    for f in os.listdir(OUT):                   # shards of an earlier run
        if f.startswith(name + ".") and f != name + ".npz":
            os.remove(os.path.join(OUT, f))
    if os.path.getsize(path) > SHARD_BYTES:
        # no file over 1 MiB in the repository: <name>.npz + <name>.1.npz, ... (tests/golden_utils.py merges them)
        import zipfile

        with zipfile.ZipFile(path) as z:
            packed = {i.filename[:-4]: i.compress_size for i in z.infolist()}
        shards, acc = [{}], 0
        for k, v in d.items():
            if shards[-1] and acc + packed[k] > SHARD_BYTES:
                shards.append({})
                acc = 0
            shards[-1][k] = v
            acc += packed[k]
        for i, s in enumerate(shards):
            np.savez_compressed(os.path.join(OUT, name + (".npz" if i == 0 else f".{i}.npz")), **s)


def main():
    tr = rs.import_reference()
    torch.set_num_threads(4)
    L = 20

    # A: item-id only, MLM train, tied full softmax   (C1/C2 structure, small dims)
    V, d, nh, nl, B = 300, 32, 2, 2, 12
    mA = build(tr, V, L, d, nh, nl, emb_default=d, seed=10)
    xA = synth_inputs(B, L, V, (), (), seed=11)
    save("xlnet_mlm_item_train", run(mA, xA, True, False, True), n_head=nh, d_model=d,
         n_layer=nl, eps=0.03, L=L, V=V + 1)
    # B: same model, eval (last item) and inference (L+1) paths
    save("xlnet_mlm_item_eval", run(mA, xA, False, True, False, with_params=False), n_head=nh, d_model=d,
         n_layer=nl, eps=0.03, L=L, V=V + 1)
    save("xlnet_mlm_item_infer", run(mA, xA, False, False, False, with_params=False), n_head=nh, d_model=d,
         n_layer=nl, eps=0.03, L=L, V=V + 1)

    # C: multi-feature concat + soft embeddings + ReLU projection + task_block (item dim 16 != d)
    cats, conts = (("category", 40), ("brand", 9)), ("price", "age")
    mC = build(tr, V, L, d, nh, nl, cats=cats, conts=conts, d_output=d,
               embedding_dims={"item_id": 16, "category": 24, "brand": 8}, seed=20)
    xC = synth_inputs(B, L, V, cats, conts, seed=21)
    save("xlnet_mlm_multi_train", run(mC, xC, True, False, True), n_head=nh, d_model=d,
         n_layer=nl, eps=0.03, L=L, V=V + 1)

    # D: CLM (XLNet-bi + CLM, as the reference's own fixtures), untied output layer
    mD = build(tr, V, L, d, nh, nl, masking="clm", emb_default=d, weight_tying=False, seed=30)
    xD = synth_inputs(B, L, V, (), (), seed=31, min_len=2)
    save("xlnet_clm_item_train", run(mD, xD, True, False, True), n_head=nh, d_model=d,
         n_layer=nl, eps=0.03, L=L, V=V + 1)
    save("xlnet_clm_item_eval", run(mD, xD, False, True, False, with_params=False), n_head=nh, d_model=d,
         n_layer=nl, eps=0.03, L=L, V=V + 1)
    save("xlnet_clm_item_infer", run(mD, xD, False, False, False, with_params=False), n_head=nh, d_model=d,
         n_layer=nl, eps=0.03, L=L, V=V + 1)

    # E: element-wise-sum aggregation + sampled softmax (tied)
    catsE = (("category", 40),)
    mE = build(tr, V, L, d, nh, 1, cats=catsE, aggregation="element-wise-sum", emb_default=d,
               sampled_softmax=True, max_n_samples=20, seed=40)
    xE = synth_inputs(B, L, V, catsE, (), seed=41)
    save("xlnet_mlm_sum_sampled_train", run(mE, xE, True, False, True), n_head=nh, d_model=d,
         n_layer=1, eps=0.03, L=L, V=V + 1, max_n_samples=20)

    # I: GPT-2 (causal LM) and BERT (masked LM) blocks through the reference's TransformerBlock
    mG = build(tr, V, L, d, nh, nl, masking="clm", emb_default=d, seed=70, arch="gpt2")
    xG = synth_inputs(B, L, V, (), (), seed=71, min_len=2)
    save("gpt2_clm_item_train", run(mG, xG, True, False, True), n_head=nh, d_model=d, n_layer=nl,
         eps=1e-5, L=L, V=V + 1)
    save("gpt2_clm_item_infer", run(mG, xG, False, False, False, with_params=False), n_head=nh, d_model=d,
         n_layer=nl, eps=1e-5, L=L, V=V + 1)
    # (one layer: BertConfig.build leaves intermediate_size at HF's 3072, so layers are large)
    mB = build(tr, V, L, d, nh, 1, emb_default=d, seed=80, arch="bert")
    xB = synth_inputs(B, L, V, (), (), seed=81)
    save("bert_mlm_item_train", run(mB, xB, True, False, True), n_head=nh, d_model=d, n_layer=1,
         eps=0.03, L=L, V=V + 1)
    save("bert_mlm_item_infer", run(mB, xB, False, False, False, with_params=False), n_head=nh, d_model=d,
         n_layer=1, eps=0.03, L=L, V=V + 1)

    # J: a per-session (non-list) categorical context feature: [B] ids -> nn.Embedding -> [B, D],
    #    broadcast over L by ConcatFeatures._expand_non_sequential_features (tabular/base.py:53-63)
    colsJ = [ColumnSchema("item_id", tags=[Tags.CATEGORICAL, Tags.ITEM_ID, Tags.LIST, Tags.ITEM],
                          int_domain=_IntDomain(0, V), value_count=_ValueCount(1, L)),
             ColumnSchema("country", tags=[Tags.CATEGORICAL], int_domain=_IntDomain(0, 17))]
    torch.manual_seed(90)
    inJ = tr.TabularSequenceFeatures.from_schema(Schema(colsJ), max_sequence_length=L, masking="mlm",
                                                 aggregation="concat", d_output=d,
                                                 embedding_dims={"item_id": 24, "country": 8})
    cfgJ = tr.XLNetConfig.build(d_model=d, n_head=nh, n_layer=1, total_seq_length=L, dropout=0.0)
    mJ = cfgJ.to_torch_model(inJ, tr.NextItemPredictionTask(weight_tying=True))
    reinit(mJ, 91)
    xJ = synth_inputs(B, L, V, (), (), seed=92)
    xJ["country"] = torch.randint(1, 18, (B,), generator=torch.Generator().manual_seed(93))
    save("xlnet_mlm_context_train", run(mJ, xJ, True, False, True), n_head=nh, d_model=d, n_layer=1,
         eps=0.03, L=L, V=V + 1)

    # F: masking-only integer fixture, many rows (lengths 1..L incl. full rows)
    Bm = 96
    msk = tr.masking.MaskedLanguageModeling(hidden_size=4, mlm_probability=0.3)
    xF = synth_inputs(Bm, L, 5000, (), (), seed=51)["item_id"]
    dF = {"in/item_id": xF.numpy()}
    with DrawRecorder() as rec:
        info = msk._compute_masked_targets(xF, training=True)
    dF["draw/bern"] = rec.bern[0].numpy()
    dF["draw/j1"] = rec.multi[0].reshape(-1).numpy()
    dF["draw/j2"] = rec.multi[1].reshape(-1).numpy()
    dF["out/mask_schema"], dF["out/masked_targets"] = info.schema.numpy(), info.targets.numpy()
    for tag, kw in (("eval_last", dict(testing=True)), ("infer", dict())):
        info = msk._compute_masked_targets(xF, training=False, **kw)
        dF[f"out/{tag}_schema"], dF[f"out/{tag}_targets"] = info.schema.numpy(), info.targets.numpy()
    msk_all = tr.masking.MaskedLanguageModeling(hidden_size=4, eval_on_last_item_seq_only=False)
    info = msk_all._compute_masked_targets(xF, training=False, testing=True)
    dF["out/eval_all_schema"], dF["out/eval_all_targets"] = info.schema.numpy(), info.targets.numpy()
    xF2 = synth_inputs(Bm, L, 5000, (), (), seed=52, min_len=2)["item_id"]
    dF["in/item_id_clm"] = xF2.numpy()
    for tag, ckw, fkw in (
        ("clm_train", {}, dict(training=True)),
        ("clm_train_last", dict(train_on_last_item_seq_only=True), dict(training=True)),
        ("clm_eval_last", {}, dict(testing=True)),
        ("clm_eval_all", dict(eval_on_last_item_seq_only=False), dict(testing=True)),
        ("clm_infer", {}, {}),
    ):
        c = tr.masking.CausalLanguageModeling(hidden_size=4, **ckw)
        info = c._compute_masked_targets(xF2, **fkw)
        dF[f"out/{tag}_schema"], dF[f"out/{tag}_targets"] = info.schema.numpy(), info.targets.numpy()
    save("masking_int", dF, mlm_probability=0.3, L=L)

    # G: ragged -> padded through the reference's pad_inputs (random ragged batch)
    from transformers4rec.torch.utils.padding import pad_batch, pad_inputs

    g = torch.Generator().manual_seed(60)
    lens = torch.randint(0, 31, (40,), generator=g)
    offs = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)])
    vals = torch.randint(1, 1000, (int(offs[-1]),), generator=g)
    fvals = torch.rand(int(offs[-1]), generator=g)
    dG = {"in/values": vals.numpy(), "in/fvalues": fvals.numpy(), "in/offsets": offs.numpy()}
    for msl in (None, 20, 64):
        o = pad_inputs({"a__values": vals, "a__offsets": offs, "f__values": fvals,
                        "f__offsets": offs}, msl)
        dG[f"out/pad_inputs_{msl}_a"] = o["a"].numpy()
        dG[f"out/pad_inputs_{msl}_f"] = o["f"].numpy()
    o = pad_batch({"a__values": vals, "a__offsets": offs}, {"a": 7})
    dG["out/pad_batch_7"] = o["a"].numpy()
    o = pad_batch({"a__values": vals, "a__offsets": offs}, {"a": 45})
    dG["out/pad_batch_45"] = o["a"].numpy()
    save("padding", dG)

    # H: log-uniform sampler distributions
    from transformers4rec.torch.model.prediction_task import LogUniformSampler

    s = LogUniformSampler(max_n_samples=20, max_id=301, min_id=1)
    save("log_uniform", {"out/dist": s.dist.numpy(), "out/unique_dist": s.unique_sampling_dist.numpy()},
         max_id=301, min_id=1, n_sample=40)

    # K: train-time input regularisers of the paper configuration
    #    (examples/t4rec_paper_experiments/t4r_paper_repro/transf_exp_main.py:71-91):
    #    pre = StochasticSwapNoise(schema), post = [TabularDropout, "layer-norm"]
    prepost_cases(tr, V, L, d, nh)
    round3_cases(tr)


# ------------------------------------------------------------------------------------------ round 3
def json_schema(path, names=None):
    """the reference's schema.json (tensorflow-metadata JSON form read by merlin_standard_lib.Schema.from_json,
    merlin_standard_lib/schema/schema.py) -> the stand-in Schema container"""
    import json

    with open(path) as f:
        js = json.load(f)
    cols = []
    for ft in js["feature"]:
        if names is not None and ft["name"] not in names:
            continue
        tags = [Tags(t) if t in {x.value for x in Tags} else t for t in ft.get("annotation", {}).get("tag", [])]
        dom = ft.get("intDomain")
        vc = ft.get("valueCount")
        cols.append(ColumnSchema(
            ft["name"], tags=tags,
            int_domain=_IntDomain(int(dom.get("min", 0)), int(dom["max"]), dom.get("isCategorical", False)) if dom else None,
            value_count=_ValueCount(int(vc.get("min", 0)), int(vc["max"])) if vc else None))
    return Schema(cols)


def ranking_metric_case(tr):
    """L: the reference's ranking metrics (torch/ranking_metric.py) on random scores, per row and aggregated
    over two update() calls -- pins the rank-based restatement (transformers4rec_amd/ranking_metric.py)"""
    from transformers4rec.torch import ranking_metric as rm
    from transformers4rec.torch.utils import torch_utils

    g = torch.Generator().manual_seed(110)
    N, V, ks = 96, 57, [1, 5, 10, 20]
    scores = torch.randn(N, V, generator=g)
    labels = torch.randint(0, V, (N,), generator=g)
    labels[:8] = scores[:8].argmax(-1)                      # some rank-0 rows
    d = {"in/scores": scores.numpy(), "in/labels": labels.numpy()}
    onehot = torch_utils.tranform_label_to_onehot(labels, V)
    for cls in (rm.NDCGAt, rm.AvgPrecisionAt, rm.RecallAt, rm.PrecisionAt, rm.DCGAt):
        m = cls(top_ks=ks, labels_onehot=True)
        name = rs.camelcase_to_snakecase(cls.__name__)
        d[f"out/rows/{name}"] = m._metric(ks, scores, onehot).numpy()
        m.reset()
        m.update(scores[:40], labels[:40])
        m.update(scores[40:], labels[40:])
        d[f"out/mean/{name}"] = m.compute().numpy()
    save("ranking_metrics", d, top_ks=ks)


def c1_cases(tr):
    """M: BASELINE configs[0] (C1): the first 100 sessions of the reference's own testing data
    (transformers4rec/data/testing/{data.parquet,schema.json}), item id only, padded / truncated to 20 by the
    reference's pad_batch, XLNet d_model 64 / 2 layers / 4 heads, MLM, tied next-item head: train (loss, logits,
    labels, every gradient), eval and inference."""
    import pyarrow.parquet as pq
    from transformers4rec.torch.utils.padding import pad_batch

    root = os.path.join(rs.REFERENCE_ROOT, "transformers4rec", "data", "testing")
    L, d, nh, nl, B = 20, 64, 4, 2, 100
    schema = json_schema(os.path.join(root, "schema.json"), names=["item_id/list"])
    col = pq.read_table(os.path.join(root, "data.parquet"), columns=["item_id/list"]).column(0).combine_chunks()
    col = col.slice(0, B)
    offs = torch.from_numpy(np.asarray(col.offsets, dtype=np.int64))
    vals = torch.from_numpy(col.values.to_numpy(zero_copy_only=False)[int(offs[0]): int(offs[-1])].astype(np.int64))
    offs = offs - offs[0]
    x = pad_batch({"item_id/list__values": vals, "item_id/list__offsets": offs}, {"item_id/list": L})
    assert x["item_id/list"].shape == (B, L)
    torch.manual_seed(120)
    inputs = tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=L, masking="mlm",
                                                    embedding_dim_default=d)
    cfg = tr.XLNetConfig.build(d_model=d, n_head=nh, n_layer=nl, total_seq_length=L, dropout=0.0)
    model = cfg.to_torch_model(inputs, tr.NextItemPredictionTask(weight_tying=True))
    reinit(model, 121)
    V = model.heads[0].body[0].categorical_module.item_embedding_table.weight.shape[0]
    meta = dict(n_head=nh, d_model=d, n_layer=nl, eps=0.03, L=L, V=V, rows=B)
    torch.manual_seed(122)
    g = torch.Generator().manual_seed(123)
    probe_cols = torch.unique(torch.cat([x["item_id/list"].reshape(-1), torch.randint(0, V, (192,), generator=g)]))

    def shrink(dd):
        """[N, V] score matrices and the [V, d] table / table gradient do not fit a small fixture: keep the columns
        (rows) of every item id of the batch + 192 random ones exactly, and fp64 reductions over the rest"""
        pr = dd.pop("out/predictions")
        dd["sel/cols"] = probe_cols.numpy()
        dd["out/predictions_sel"] = pr[:, probe_cols.numpy()]
        dd["out/predictions_lse"] = torch.logsumexp(torch.from_numpy(pr).double(), -1).numpy()
        dd["out/predictions_rowsum"] = pr.astype(np.float64).sum(-1)
        dd["out/predictions_argmax"] = pr.argmax(-1)
        for k in list(dd):
            if k.startswith("g/") and dd[k].shape == (V, d):
                gtab = dd.pop(k)
                dd["gsel/" + k[2:]] = gtab[probe_cols.numpy()]
                dd["gsum/" + k[2:]] = gtab.astype(np.float64).sum(0)
                dd["gabs/" + k[2:]] = np.abs(gtab.astype(np.float64)).sum(0)
        return dd

    dd = shrink(run(model, x, True, False, True, with_params=False))
    # the wire form of the same rows (what data.parquet holds, untruncated) and the schema.json entry of the column:
    # the GPU test writes them back to a parquet / json pair and feeds them through ParquetSessionLoader + from_json
    dd["in_ragged/item_id/list__values"], dd["in_ragged/item_id/list__offsets"] = vals.numpy(), offs.numpy()
    import json

    with open(os.path.join(root, "schema.json")) as f:
        ent = [ft for ft in json.load(f)["feature"] if ft["name"] == "item_id/list"]
    dd["meta/schema_json"] = np.asarray(json.dumps({"feature": ent}))
    # parameters: everything but the [V, d] table is stored; the table (13 MB of noise) is stored as its RECIPE --
    # reinit() draws every parameter from Generator(reinit_seed) in named_parameters order -- which the test
    # replays and checks against the stored parameters before trusting the table it produces
    seen = set()
    for k, v in model.state_dict().items():
        if v.data_ptr() in seen:
            continue
        seen.add(v.data_ptr())
        if tuple(v.shape) == (V, d):
            dd["sel/table_rows"] = v.detach().numpy()[probe_cols.numpy()].copy()
            dd["meta/table_key"] = np.asarray(k)
        else:
            dd["p/" + k] = v.detach().numpy().copy()
    named = list(model.named_parameters())
    dd["meta/param_order"] = np.asarray([n for n, _ in named])
    dd["meta/param_shapes"] = np.asarray([",".join(str(int(z)) for z in p.shape) for _, p in named])
    dd["meta/reinit_seed"] = np.asarray(121)
    save("c1_yoochoose_train", dd, **meta)
    save("c1_yoochoose_eval", shrink(run(model, x, False, True, False, with_params=False)), **meta)
    save("c1_yoochoose_infer", shrink(run(model, x, False, False, False, with_params=False)), **meta)


def embedding_bag_cases(tr):
    """N: EmbeddingFeatures' EmbeddingBag branch (features/embedding.py:86-93, 229-240, 260-273): per-row bags as
    2-D [B, K] ids, ragged (values, offsets) bags and 1-D [B] ids, combiners mean and sum; outputs and the table
    gradients of  sum_f <out_f, c_f>  with fixed random c_f."""
    from transformers4rec.torch.features.embedding import EmbeddingFeatures, FeatureConfig, TableConfig

    g = torch.Generator().manual_seed(130)
    B = 37
    for comb in ("mean", "sum"):
        cfgs = {"genres": FeatureConfig(TableConfig(50, 24, name="genres", combiner=comb)),
                "tags": FeatureConfig(TableConfig(400, 64, name="tags", combiner=comb)),
                "country": FeatureConfig(TableConfig(19, 8, name="country", combiner=comb))}
        torch.manual_seed(131)
        mod = EmbeddingFeatures(cfgs)
        with torch.no_grad():
            for p in mod.parameters():
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
        genres = torch.randint(0, 50, (B, 5), generator=g)             # fixed-width bags, padding id 0 included
        lens = torch.randint(0, 9, (B,), generator=g)                   # ragged bags, some EMPTY
        lens[0], lens[B - 1] = 0, 3
        offs = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)])[:-1]
        tvals = torch.randint(0, 400, (int(lens.sum()),), generator=g)
        country = torch.randint(0, 19, (B,), generator=g)
        # 2-D and 1-D ids run through the UNMODIFIED module.  The (values, offsets) tuple branch (:229-236) cannot: it
        # calls `self.embedding_tables[name](values, offsets[:, 0])`, but EmbeddingBagWrapper.forward(self, input,
        # **kwargs) (:260-273) accepts no positional offsets -> TypeError in the reference as shipped (and no reference
        # test covers it).  The fixture follows the evident intent of that line: torch.nn.EmbeddingBag.forward(table,
        # values.squeeze(-1), offsets[:, 0]) on the module's own table.
        out = mod({"genres": genres, "country": country})
        try:
            mod({"tags": (tvals.unsqueeze(-1), offs.unsqueeze(-1))})
            raise AssertionError("the reference's tuple branch ran: regenerate this fixture through it")
        except TypeError:
            pass
        out["tags"] = torch.nn.EmbeddingBag.forward(mod.embedding_tables["tags"], tvals.unsqueeze(-1).squeeze(-1),
                                                    offs.unsqueeze(-1)[:, 0])
        c = {k: torch.randn(v.shape, generator=g) for k, v in out.items()}
        sum((out[k] * c[k]).sum() for k in out).backward()
        d = {"in/genres": genres.numpy(), "in/tags_values": tvals.numpy(), "in/tags_offsets": offs.numpy(),
             "in/country": country.numpy()}
        for k in out:
            d["out/" + k] = out[k].detach().numpy()
            d["c/" + k] = c[k].numpy()
            d["p/" + k] = mod.embedding_tables[k].weight.detach().numpy().copy()
            d["g/" + k] = mod.embedding_tables[k].weight.grad.numpy().copy()
        save(f"embedding_bag_{comb}", d, combiner=comb, B=B)


def round3_cases(tr):
    ranking_metric_case(tr)
    c1_cases(tr)
    embedding_bag_cases(tr)


class SwapRecorder:
    """Records every StochasticSwapNoise.augment call (input, padding mask, bernoulli, randperm,
    output) in call order while the reference runs."""

    def __init__(self, tr):
        self.cls, self.calls = tr.StochasticSwapNoise, []

    def __enter__(self):
        self._aug, self._b, self._p = self.cls.augment, torch.bernoulli, torch.randperm
        cur = {}

        rec = self

        def augment(ssn, x, mask=None):
            cur.clear()
            b0, p0 = torch.bernoulli, torch.randperm   # whatever is installed now (e.g. DrawRecorder)

            def bern(*a, **k):
                r = rec._b(*a, **k)
                cur.setdefault("bern", r.clone())
                return r

            def perm(*a, **k):
                r = rec._p(*a, **k)
                cur.setdefault("perm", r.clone())
                return r

            torch.bernoulli, torch.randperm = bern, perm
            try:
                out = rec._aug(ssn, x, mask)
            finally:
                torch.bernoulli, torch.randperm = b0, p0
            rec.calls.append(dict(x=x.clone(), out=out.clone(), **cur))
            return out

        self.cls.augment = augment
        return self

    def __exit__(self, *exc):
        self.cls.augment = self._aug


def prepost_cases(tr, V, L, d, nh):
    B = 10
    cats, conts = (("category", 40), ("brand", 9)), ("price",)
    feats = ["item_id", "category", "brand", "price"]
    schema = make_schema(V, L, cats, conts)
    for name, post_fn, agg, dims in (
        ("xlnet_mlm_prepost_concat_train", lambda: [tr.TabularDropout(0.25), "layer-norm"], "concat",
         {"item_id": 16, "category": 24, "brand": 8}),
        ("xlnet_mlm_prepost_sum_train", lambda: ["layer-norm", tr.TabularDropout(0.25)], "element-wise-sum-item-multi",
         None),
    ):
        conts_k = conts if agg == "concat" else ()
        schema_k = schema if agg == "concat" else make_schema(V, L, cats, ())
        ssn = tr.StochasticSwapNoise(pad_token=0, replacement_prob=0.3, schema=schema_k)
        kw = dict(max_sequence_length=L, masking="mlm", aggregation=agg, pre=[ssn], post=post_fn())
        if agg == "concat":
            kw.update(d_output=d, continuous_soft_embeddings=True, embedding_dims=dims)
        else:
            kw.update(embedding_dim_default=d)
        torch.manual_seed(100)
        inp = tr.TabularSequenceFeatures.from_schema(schema_k, **kw)
        cfg = tr.XLNetConfig.build(d_model=d, n_head=nh, n_layer=1, total_seq_length=L, dropout=0.0)
        model = cfg.to_torch_model(inp, tr.NextItemPredictionTask(weight_tying=(agg != "concat")))
        reinit(model, 101)
        model.train()   # the regularisers follow nn.Module.training (transformations.py:59-60)
        # (XLNetConfig dropout = 0, so the transformer and the head stay deterministic)
        x = synth_inputs(B, L, V, cats, conts_k, seed=102)
        cat_mod = inp.categorical_module
        drop_mod = [t for t in cat_mod.post if isinstance(t, tr.TabularDropout)][0]
        keep = {}

        def hook(mod, args, out):
            for k, v in out.items():
                keep[k] = (v != 0).to(torch.uint8)   # |embedding| > 0 almost surely; checked below

        hd = drop_mod.register_forward_hook(hook)
        torch.manual_seed(103)
        with SwapRecorder(tr) as sw:
            dd = run(model, x, True, False, True)
        hd.remove()
        # augment is called once per input feature per module, modules in to_merge order
        n_in = len(x)
        mods = list(inp.to_merge.keys())
        assert len(sw.calls) == n_in * len(mods), (len(sw.calls), n_in, mods)
        for mi, mname in enumerate(mods):
            for fi, fname in enumerate(x.keys()):
                c = sw.calls[mi * n_in + fi]
                assert torch.equal(c["x"], x[fname])
                dd[f"draw/ssn_bern/{mname}/{fname}"] = c["bern"].numpy().astype(np.uint8)
                dd[f"draw/ssn_perm/{mname}/{fname}"] = c["perm"].numpy()
                dd[f"out/ssn/{mname}/{fname}"] = c["out"].numpy()
        for k, v in keep.items():
            frac = float(v.float().mean())
            assert 0.6 < frac < 0.9, (k, frac)
            dd[f"draw/post_keep/{k}"] = v.numpy()
        dd["out/item_seq"] = cat_mod.item_seq.numpy()
        save(name, dd, n_head=nh, d_model=d, n_layer=1, eps=0.03, L=L, V=V + 1, ssn_p=0.3, post_drop_p=0.25)


# ------------------------------------------------------------------------------------------ round 6
def long_cases(tr):
    """Sequences beyond one wave of the attention kernels (total_seq_length 100: the reference takes any length,
    config/transformer.py:432-482): XLNet MLM train / eval / inference (the inference pass runs the body on L + 1 = 101
    positions, masking.py:406-418), XLNet CLM train; GPT-2 CLM and BERT MLM train at total_seq_length 150."""
    L, V, d, nh, nl, B = 100, 300, 32, 2, 2, 6
    m = build(tr, V, L, d, nh, nl, emb_default=d, seed=70)
    x = synth_inputs(B, L, V, (), (), seed=71, min_len=40)
    save("xlnet_mlm_long_train", run(m, x, True, False, True), n_head=nh, d_model=d, n_layer=nl, eps=0.03, L=L, V=V + 1)
    save("xlnet_mlm_long_eval", run(m, x, False, True, False, with_params=False), n_head=nh, d_model=d, n_layer=nl, eps=0.03,
         L=L, V=V + 1)
    save("xlnet_mlm_long_infer", run(m, x, False, False, False, with_params=False), n_head=nh, d_model=d, n_layer=nl, eps=0.03,
         L=L, V=V + 1)
    mD = build(tr, V, L, d, nh, nl, masking="clm", emb_default=d, seed=72)
    xD = synth_inputs(B, L, V, (), (), seed=73, min_len=40)
    save("xlnet_clm_long_train", run(mD, xD, True, False, True), n_head=nh, d_model=d, n_layer=nl, eps=0.03, L=L, V=V + 1)
    # GPT-2 (causal) and BERT beyond 128 positions (the LDS attention kernels' bound), head width 24 (d_model 48, two heads)
    L, d, B = 150, 48, 4
    mG = build(tr, V, L, d, nh, 1, masking="clm", emb_default=d, seed=74, arch="gpt2")
    xG = synth_inputs(B, L, V, (), (), seed=75, min_len=100)
    save("gpt2_clm_long_train", run(mG, xG, True, False, True), n_head=nh, d_model=d, n_layer=1, eps=1e-5, L=L, V=V + 1)
    mB = build(tr, V, L, d, nh, 1, emb_default=d, seed=76, arch="bert")
    xB = synth_inputs(B, L, V, (), (), seed=77, min_len=100)
    save("bert_mlm_long_train", run(mB, xB, True, False, True), n_head=nh, d_model=d, n_layer=1, eps=0.03, L=L, V=V + 1)


if __name__ == "__main__":
    if "--round3" in sys.argv:          # only the fixtures added in round 3 (the others are unchanged)
        torch.set_num_threads(4)
        round3_cases(rs.import_reference())
    elif "--long" in sys.argv:          # only the fixtures added in round 6
        torch.set_num_threads(4)
        long_cases(rs.import_reference())
    else:
        main()
        long_cases(rs.import_reference())
