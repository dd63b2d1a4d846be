"""Input block: host-side mirror of the reference's
  SequenceEmbeddingFeatures / EmbeddingFeatures   transformers4rec/torch/features/{sequence.py:43-94, embedding.py:51-276}
  SoftEmbeddingFeatures / SoftEmbedding           features/embedding.py:280-410, 517-556
  TabularSequenceFeatures                         features/sequence.py:97-296
with the same constructor arguments for the hot path, attribute contract (`masking`,
`item_id`, `item_embedding_table`, `categorical_module.item_seq`, `to_merge[...]`,
`projection_module`) and state_dict names.  All arithmetic runs in
csrc/embedding.hip / gemm_f32.hip through one fused autograd function.
"""
import functools
import math
import os
from typing import Dict, Optional

import torch
from torch import nn

from . import ops
from .transformations import TabularDropout, TabularLayerNorm, parse_post, parse_pre
from .masking import MaskSequence, _grad_buf, parse_masking
from .schema import Tags, categorical_cardinalities

# table-gradient scatter: stable sort by row id (done in the forward pass: it depends on the ids only) + segmented sum,
# deterministic, one owner per row (csrc/embedding_sorted.hip).  The fp32-row-atomics scatter (ops.embedding_bwd) is
# still in the C ABI for callers that want it; the module path does not use it.


def _table_scatter(ctx, name, grad_rows, ids_f, tab, col, dim, padding_idx):
    """d table += gradient rows of one feature.  grad_rows [n_lookups * ids_div, W]"""
    ids_div = grad_rows.numel() // grad_rows.shape[-1] // ids_f.numel()
    sink = getattr(tab, "_t4r_sparse_sink", None)
    if sink is not None:            # data-parallel row-sparse exchange (distributed.SparseRowExchange)
        sink.add(tab, ids_f, grad_rows, col, dim, ids_div, padding_idx)
        return
    srt = ctx.sorted_ids.get(name)
    if srt is None:
        srt = ops.sort_ids(ids_f, tab.shape[0], padding_idx)
    ops.embedding_bwd_sorted(grad_rows, srt[0], srt[1], _grad_buf(tab), col, dim, ids_div)


def _sort_ids_forward(ids, rows, padding_idx):
    """the forward-pass sort (it feeds only the backward), on the caller's stream.  (Rounds 3-4 ran it on a side stream; it
    was worth nothing at BASELINE configs[1] -- 2.834 vs 2.847 ms per step -- and a training step must not drive more than
    FOUR streams: caller + two weight-gradient streams + the collective's, DESIGN.md section 6.  Removed in round 6.)"""
    return ops.sort_ids(ids, rows, padding_idx)


def _sort_ids_forward_multi(ids_list, rows_list, padding_idx):
    """_sort_ids_forward for the F tables of one input block as ONE device sort -> [(keys, perm)] per table"""
    return ops.sort_ids_multi(ids_list, rows_list, [padding_idx] * len(ids_list))


class EmbeddingTable(nn.Module):
    """nn.Embedding-shaped parameter holder (`weight`, num_embeddings, embedding_dim, padding_idx)."""

    def __init__(self, num_embeddings, embedding_dim, padding_idx=None, std=0.05):
        super().__init__()
        self.num_embeddings, self.embedding_dim, self.padding_idx = num_embeddings, embedding_dim, padding_idx
        self.weight = nn.Parameter(torch.empty(num_embeddings, embedding_dim))
        # TableConfig default initializer normal_(0, 0.05) runs AFTER nn.Embedding's padding row
        # zero-fill (features/sequence.py:75-81; embedding.py:460-464): row 0 is random, not zero.
        nn.init.normal_(self.weight, mean=0.0, std=std)

    def extra_repr(self):
        return f"{self.num_embeddings}, {self.embedding_dim}, padding_idx={self.padding_idx}"


class _Linear(nn.Module):
    """torch.nn.Linear-shaped parameter holder with the same default init."""

    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.empty(out_features)) if bias else None
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if bias:
            bound = 1 / math.sqrt(in_features) if in_features > 0 else 0
            nn.init.uniform_(self.bias, -bound, bound)


class _LayerNormParams(nn.Module):
    def __init__(self, dim, eps=1e-5):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim))
        self.bias = nn.Parameter(torch.zeros(dim))


class SoftEmbedding(nn.Module):
    """reference features/embedding.py:517-556: `embedding_table` [K, D] + `projection_layer` Linear(1, K)"""

    def __init__(self, num_embeddings, embeddings_dim):
        super().__init__()
        self.embedding_table = EmbeddingTable(num_embeddings, embeddings_dim)
        self.projection_layer = _Linear(1, num_embeddings)


class _SeqEmbeddingsFn(torch.autograd.Function):
    """the lookups of a stand-alone SequenceEmbeddingFeatures call: one concatenating gather (t4r_seq_features_fwd) into
    [B, L, sum(dims)]; backward: each table's column block through the deterministic sorted scatter into `.grad`, as everywhere
    on this path."""

    @staticmethod
    def forward(ctx, anchor, mod, names, ids, err):
        B, L = ids[0].shape
        feats, col = [], 0
        for n, i in zip(names, ids):
            tab = mod.embedding_tables[n].weight
            feats.append(dict(kind=0, input=i, table=tab.detach(), dim=tab.shape[1], col=col, rows=tab.shape[0]))
            col += tab.shape[1]
        ctx.mod, ctx.names, ctx.ids, ctx.sorted_ids = mod, names, ids, {}
        return ops.seq_features_fwd(feats, "concat", B, L, L, col, err_flag=err)

    @staticmethod
    def backward(ctx, dy):
        d2 = dy.contiguous().view(-1, dy.shape[-1])
        col = 0
        for n, i in zip(ctx.names, ctx.ids):
            tab = ctx.mod.embedding_tables[n].weight
            if tab.requires_grad:
                _table_scatter(ctx, n, d2, i.view(-1), tab, col, tab.shape[1], ctx.mod.padding_idx)
            col += tab.shape[1]
        return None, None, None, None, None


class SequenceEmbeddingFeatures(nn.Module):
    """Categorical sequence features; holds `embedding_tables` and the stateful `item_seq`.  Inside a TabularSequenceFeatures
    the block's one kernel does the lookups; called on its own (a post-context module, experimental.PostContextFusion),
    forward(inputs) returns {name: [B, L, dim]} (aggregation=None) or their concatenation in sorted-name order
    (aggregation="concat", tabular/aggregation.py:35-47)."""

    def __init__(self, table_sizes: Dict[str, tuple], item_id: Optional[str] = None, padding_idx: int = 0,
                 pre=None, post=None, aggregation: Optional[str] = None):
        super().__init__()
        if aggregation not in (None, "concat"):
            raise NotImplementedError("SequenceEmbeddingFeatures on the HIP path aggregates with None or 'concat'")
        self.aggregation = aggregation
        self._err = None
        self.item_id = item_id
        self.padding_idx = padding_idx
        self.embedding_tables = nn.ModuleDict(
            {n: EmbeddingTable(v, d, padding_idx=padding_idx) for n, (v, d) in table_sizes.items()})
        self.item_seq = None
        # pre / post transformations (TabularModule, tabular/base.py:226-283); state-dict names as the
        # reference: `_post.<i>.feature_layer_norm.<feature>.{weight,bias}`
        self._pre = parse_pre(pre)
        self._post = parse_post(post, {n: d for n, (v, d) in table_sizes.items()})

    @property
    def pre(self):
        return self._pre

    @property
    def post(self):
        return self._post

    @property
    def item_embedding_table(self):
        assert self.item_id is not None
        return self.embedding_tables[self.item_id]

    def item_ids(self, inputs):
        return inputs[self.item_id]

    def forward(self, inputs, **kwargs):
        """stand-alone lookups of the features present in `inputs` ([B, L] int64 ids each)"""
        if self._pre is not None or self._post is not None:
            raise NotImplementedError("pre / post transformations of a stand-alone SequenceEmbeddingFeatures are off the hot path")
        names = [n for n in sorted(self.embedding_tables) if n in inputs]
        if not names:
            return {}
        ids = [inputs[n].contiguous() for n in names]
        if any(i.dim() != 2 or i.shape != ids[0].shape for i in ids):
            raise ValueError("SequenceEmbeddingFeatures: every feature must be [B, L] ids of one shape")
        dev = self.embedding_tables[names[0]].weight.device
        if self._err is None or self._err.device != dev:
            self._err = torch.zeros(1, dtype=torch.int32, device=dev)
        if self.item_id and self.item_id in inputs:
            self.item_seq = self.item_ids(inputs)
        anchor = self.embedding_tables[names[0]].weight
        if self.aggregation == "concat":
            return _SeqEmbeddingsFn.apply(anchor, self, names, ids, self._err)
        return {n: _SeqEmbeddingsFn.apply(self.embedding_tables[n].weight, self, [n], [i], self._err) for n, i in zip(names, ids)}

    def forward_output_size(self, input_sizes=None):
        return {n: torch.Size([-1, -1, t.embedding_dim]) for n, t in self.embedding_tables.items()}

    def output_size(self, input_size=None):
        sizes = self.forward_output_size()
        if self.aggregation != "concat":
            return sizes
        return torch.Size([-1, -1, sum(s[-1] for s in sizes.values())])


class TableConfig:
    """features/embedding.py:416-460: vocabulary_size, dim, initializer, combiner ("mean" | "sum" | "sqrtn"), name"""

    def __init__(self, vocabulary_size: int, dim: int, initializer=None, combiner: str = "mean", name: Optional[str] = None):
        if not isinstance(vocabulary_size, int) or vocabulary_size < 1:
            raise ValueError("Invalid vocabulary_size {}.".format(vocabulary_size))
        if not isinstance(dim, int) or dim < 1:
            raise ValueError("Invalid dim {}.".format(dim))
        if combiner not in ("mean", "sum", "sqrtn"):
            raise ValueError("Invalid combiner {}".format(combiner))
        if initializer is not None and not callable(initializer):
            raise ValueError("initializer must be callable if specified.")
        self.vocabulary_size, self.dim, self.combiner, self.name = vocabulary_size, dim, combiner, name
        # features/embedding.py:460-464: no initializer means normal_(mean 0, std 0.05), always applied by
        # table_to_embedding_module -- bag tables start at std 0.05 too, not at EmbeddingBag's N(0, 1)
        # (a functools.partial, as the reference: a lambda here made torch.save(model) / pickle fail)
        self.initializer = functools.partial(nn.init.normal_, mean=0.0, std=0.05) if initializer is None else initializer

    def __repr__(self):
        return (f"TableConfig(vocabulary_size={self.vocabulary_size!r}, dim={self.dim!r}, "
                f"combiner={self.combiner!r}, name={self.name!r})")


class FeatureConfig:
    """features/embedding.py:391-413"""

    def __init__(self, table: TableConfig, max_sequence_length: int = 0, name: Optional[str] = None):
        self.table, self.max_sequence_length, self.name = table, max_sequence_length, name


class _BagTable(nn.Module):
    """EmbeddingBagWrapper-shaped parameter holder (`weight`, `mode`).  The TableConfig's initializer -- normal_(0, 0.05)
    when the user gave none (features/embedding.py:460-464) -- always runs after construction (:86-93); built without one
    (direct use), the same N(0, 0.05) default as `EmbeddingTable`."""

    def __init__(self, num_embeddings, embedding_dim, mode="mean", initializer=None):
        super().__init__()
        self.num_embeddings, self.embedding_dim, self.mode = num_embeddings, embedding_dim, mode
        self.weight = nn.Parameter(torch.empty(num_embeddings, embedding_dim))
        nn.init.normal_(self.weight, mean=0.0, std=0.05)
        if initializer is not None:
            initializer(self.weight)

    def extra_repr(self):
        return f"{self.num_embeddings}, {self.embedding_dim}, mode={self.mode!r}"


class _EmbeddingBagsFn(torch.autograd.Function):
    """all bag lookups of one EmbeddingFeatures call.  forward: `t4r_embedding_bag_fwd` per feature, into its own
    [B, dim] tensor or (concat) into its columns of ONE [B, W] buffer; backward: per-lookup gradient rows
    (`t4r_embedding_bag_bwd_rows`) summed into the table by the deterministic sorted scatter, or handed to the
    data-parallel row-sparse sink.  Table gradients go straight into `.grad`, as everywhere on this path."""

    @staticmethod
    def forward(ctx, anchor, tables, lookups, concat, err):
        # lookups: [(values int64, offsets int64 | None, combiner)] aligned with `tables`
        B = lookups[0][1].numel() if lookups[0][1] is not None else lookups[0][0].shape[0]
        cols, c = [], 0
        for t in tables:
            cols.append(c)
            c += t.shape[1] if concat else 0
        wide = torch.empty((B, c), device=anchor.device, dtype=torch.float32) if concat else None
        outs, saved = [], []
        for t, (vals, offs, comb), col in zip(tables, lookups, cols):
            vals = vals.contiguous()
            offs = None if offs is None else offs.contiguous()
            outs.append(ops.embedding_bag_fwd(t.detach(), vals, offs, comb, out=wide, col=col, err_flag=err))
            saved.append((vals, offs, comb, 0 if offs is not None else vals.numel() // max(vals.shape[0], 1), col))
        ctx.tables, ctx.saved, ctx.concat = tables, saved, concat
        return (wide,) if concat else tuple(outs)

    @staticmethod
    def backward(ctx, *douts):
        for i, (tab, (vals, offs, comb, fixed_k, col)) in enumerate(zip(ctx.tables, ctx.saved)):
            dout = douts[0] if ctx.concat else douts[i]
            if dout is None:
                continue
            rows = ops.embedding_bag_bwd_rows(dout.contiguous(), vals.numel(), tab.shape[1], offs, fixed_k, comb, col=col)
            ids = vals.view(-1)
            sink = getattr(tab, "_t4r_sparse_sink", None)
            if sink is not None:
                sink.add_rows(tab, ids, rows, padding_idx=-1)
            else:
                ops.scatter_rows_sorted(_grad_buf(tab), ids, rows, padding_idx=-1)
        return None, None, None, None, None


class EmbeddingFeatures(nn.Module):
    """Drop-in for tr.EmbeddingFeatures (features/embedding.py:43-249), the NON-sequential categorical module whose
    tables are EmbeddingBags: per feature `inputs[name]` is

      * int64 [B]              -> bags of one id                       -> [B, dim]
      * int64 [B, K]           -> one bag of K ids per row (id 0 counts) -> [B, dim]
      * (values, offsets)      -> ragged bags; values [n] or [n, 1], offsets [B] or [B, 1] (the Merlin loader's
                                  sparse form, :229-236)                 -> [B, dim]

    combined with the table's `combiner`.  ("sqrtn" = sum / sqrt(n) is what TableConfig documents; the reference's
    torch.nn.EmbeddingBag rejects that mode at run time, and its tuple branch raises a TypeError as shipped -- the
    fixtures tests/golden/embedding_bag_*.npz record what the reference does compute.)
    forward returns {name: [B, dim]} (aggregation=None) or their concatenation in sorted-name order
    (aggregation="concat", tabular/aggregation.py:35-47).  state_dict names: `embedding_tables.<name>.weight`."""

    def __init__(self, feature_config: Dict[str, FeatureConfig], item_id: Optional[str] = None, pre=None, post=None,
                 aggregation: Optional[str] = None, schema=None):
        super().__init__()
        if pre is not None or post is not None:
            raise NotImplementedError("pre / post transformations on EmbeddingFeatures are off the hot path")
        if aggregation not in (None, "concat"):
            raise NotImplementedError("EmbeddingFeatures on the HIP path aggregates with None or 'concat'")
        self.item_id, self.feature_config, self.aggregation, self.schema = item_id, feature_config, aggregation, schema
        tables = {}
        for name, feature in feature_config.items():
            t = feature.table
            if name not in tables:
                tables[name] = _BagTable(t.vocabulary_size, t.dim, t.combiner, t.initializer)
        self.embedding_tables = nn.ModuleDict(tables)
        self.item_seq = None
        self._err = None

    @classmethod
    def from_schema(cls, schema, embedding_dims=None, embedding_dim_default: int = 64, infer_embedding_sizes=False,
                    infer_embedding_sizes_multiplier: float = 2.0, embeddings_initializers=None,
                    combiner: str = "mean", tags=None, item_id=None, automatic_build=True,
                    max_sequence_length=None, aggregation=None, pre=None, post=None, **kwargs):
        """features/embedding.py:95-221"""
        if infer_embedding_sizes:
            raise NotImplementedError("infer_embedding_sizes is off the hot path: pass embedding_dims")
        if tags:
            schema = schema.select_by_tag(tags)
        ids = schema.select_by_tag(Tags.ITEM_ID)
        if not item_id and len(ids) > 0:
            if len(ids) > 1:
                raise ValueError("Multiple columns with tag ITEM_ID found. Please specify the item_id column name.")
            item_id = ids.column_names[0]
        embedding_dims = embedding_dims or {}
        inits = embeddings_initializers or {}
        cfg = {name: FeatureConfig(TableConfig(card, embedding_dims.get(name, embedding_dim_default),
                                               initializer=inits.get(name), combiner=combiner, name=name))
               for name, card in categorical_cardinalities(schema).items()}
        if not cfg:
            return None
        return cls(cfg, item_id=item_id, pre=pre, post=post, aggregation=aggregation, schema=schema)

    @property
    def item_embedding_table(self):
        assert self.item_id is not None
        return self.embedding_tables[self.item_id]

    def item_ids(self, inputs):
        return inputs[self.item_id]

    def check_ids(self):
        """raises if a lookup since the last call saw an id outside its table (one host sync)"""
        if self._err is not None and int(self._err.item()) != 0:
            self._err.zero_()
            raise IndexError("EmbeddingFeatures: id outside [0, vocabulary_size)")

    def forward(self, inputs, **kwargs):
        names = [n for n in (sorted(self.feature_config) if self.aggregation == "concat" else self.feature_config)
                 if n in inputs]
        if not names:
            return {}
        tables, lookups = [], []
        for name in names:
            val = inputs[name]
            tab = self.embedding_tables[name]
            if isinstance(val, tuple):
                values, offsets = val
                values = values.reshape(-1)
                offsets = offsets[:, 0] if offsets.ndim == 2 else offsets
            else:
                values, offsets = val, None
                if val.ndim not in (1, 2):
                    raise ValueError(f"EmbeddingFeatures: {name} must be [B], [B, K] or a (values, offsets) tuple")
            tables.append(tab.weight)
            lookups.append((values, offsets, tab.mode))
        dev = tables[0].device
        if self._err is None or self._err.device != dev:
            self._err = torch.zeros(1, dtype=torch.int32, device=dev)
        concat = self.aggregation == "concat"
        outs = _EmbeddingBagsFn.apply(tables[0], tables, lookups, concat, self._err)
        if self.item_id:
            self.item_seq = self.item_ids(inputs)
        return outs[0] if concat else dict(zip(names, outs))

    def forward_output_size(self, input_sizes=None):
        return {name: torch.Size([-1, f.table.dim]) for name, f in self.feature_config.items()}


class _FeaturePost(nn.Module):
    def __init__(self, dims: Dict[str, int]):
        super().__init__()
        self.feature_layer_norm = nn.ModuleDict({n: _LayerNormParams(d) for n, d in dims.items()})


class SoftEmbeddingFeatures(nn.Module):
    """Continuous features through SoftEmbedding (+ per-feature LayerNorm in `post`)."""

    def __init__(self, table_sizes: Dict[str, tuple], layer_norm: bool = True, pre=None, post=None):
        super().__init__()
        if post is not None and not layer_norm:
            raise NotImplementedError("post transformations on soft embeddings other than the built-in "
                                      "layer norm are off the hot path")
        self._pre = parse_pre(pre)   # `post` is replaced by the LayerNorm when layer_norm=True (embedding.py:306-309)
        self.embedding_tables = nn.ModuleDict({n: SoftEmbedding(k, d) for n, (k, d) in table_sizes.items()})
        self.post = _FeaturePost({n: d for n, (k, d) in table_sizes.items()}) if layer_norm else None


class ContinuousFeatures(nn.Module):
    """Continuous sequence features passed through as width-1 columns
    (features/continuous.py:60-63: unsqueeze(-1)); no parameters."""

    def __init__(self, names, pre=None, post=None):
        super().__init__()
        self.names = list(names)
        self._pre = parse_pre(pre)
        self._post = parse_post(post, {n: 1 for n in self.names})   # LayerNorm skips dim-1 features
        self.embedding_tables = nn.ModuleDict()
        self.post = None


class _AsTabular(nn.Module):
    """the parameter-free marker that names a block's output (reference tabular/base.py: AsTabular)"""

    def __init__(self, output_name):
        super().__init__()
        self.output_name = output_name

    def extra_repr(self):
        return repr(self.output_name)


CONTINUOUS_PROJECTION = "continuous_projection"


class ContinuousProjection(nn.Sequential):
    """The continuous module after `project_continuous_features(dims)` (reference features/tabular.py:90-117,
    features/sequence.py:271-284): SequentialBlock(ContinuousFeatures(aggregation="concat"), MLPBlock(dims),
    AsTabular("continuous_projection")).  The C continuous columns, in sorted-name order, go through ReLU(Linear) layers
    (block/mlp.py:68-143: no dropout, no normalisation) and come out as ONE feature, `continuous_projection`, of width
    dims[-1].  Members and state-dict names are the reference's: [0] the parameter-free ContinuousFeatures, [1] a sequence of
    one-Linear sequences (`1.<i>.0.{weight,bias}`, torch.nn.Linear's default init), [2] the marker.  The first layer runs in
    csrc/cont_proj.hip from the separate column tensors, the others on the general GEMM."""

    def __init__(self, continuous, dims):
        if not isinstance(continuous, ContinuousFeatures):
            raise NotImplementedError("continuous_projection projects plain ContinuousFeatures; soft embeddings fed into the "
                                      "projection (continuous_soft_embeddings=True) are off the hot path")
        if not continuous.names:
            raise ValueError("continuous_projection needs at least one continuous column")
        if continuous._post is not None:
            raise NotImplementedError("post transformations on a continuous module with continuous_projection are off the hot "
                                      "path")
        dims = [dims] if isinstance(dims, int) else list(dims)
        if not dims or any(not isinstance(d, int) or d < 1 for d in dims):
            raise ValueError(f"continuous_projection takes an int or a non-empty list of positive ints, got {dims!r}")
        C = len(continuous.names)
        if not 1 <= C <= 64 or not 1 <= dims[0] <= 1024:
            raise NotImplementedError(f"continuous_projection: {C} columns into {dims[0]} units is outside what the first-layer "
                                      "kernel takes (1..64 columns, 1..1024 units)")
        sizes = [C] + dims
        mlp = nn.Sequential(*[nn.Sequential(_Linear(i, o)) for i, o in zip(sizes[:-1], sizes[1:])])
        super().__init__(continuous, mlp, _AsTabular(CONTINUOUS_PROJECTION))
        self.dims = dims

    @property
    def names(self):
        """the raw continuous columns in the order the first layer's weight columns follow"""
        return sorted(self[0].names)

    @property
    def layers(self):
        return [dense[0] for dense in self[1]]

    @property
    def output_dim(self):
        return self.dims[-1]

    @property
    def _pre(self):
        return self[0]._pre

    @property
    def embedding_tables(self):
        return self[0].embedding_tables


def _cont_proj_fwd(cont, inputs, B, L):
    """the rows [B * L, dims[-1]] of the `continuous_projection` feature -> (rows, record for _cont_proj_bwd)"""
    xs, flags = [], []
    for n in cont.names:
        x = inputs[n].contiguous().float()
        if x.ndim == 1 and x.shape[0] == B:
            flags.append(True)          # a per-session column, broadcast over L (reference: tabular/base.py:53-63)
        elif tuple(x.shape) == (B, L):
            flags.append(False)
        else:
            raise ValueError(f"continuous feature {n!r}: expected [{B}, {L}] or [{B}], got {tuple(x.shape)}")
        xs.append(x)
    layers = cont.layers
    acts = [ops.cont_proj_fwd(xs, flags, layers[0].weight.detach(), layers[0].bias.detach(), T=B * L)]
    for lin in layers[1:]:
        acts.append(ops.gemm(acts[-1], lin.weight.detach(), False, True, bias=lin.bias.detach(), epilogue=ops.EPI_BIAS_RELU))
    return acts[-1], dict(xs=xs, flags=flags, acts=acts)


def _cont_proj_bwd(cont, rec, d2, col):
    """parameter gradients of the projection MLP from columns [col, col + dims[-1]) of the aggregate's gradient d2 [B * L, W];
    d2 is read only"""
    layers, acts = cont.layers, rec["acts"]
    g, gcol = d2, col
    for i in range(len(layers) - 1, 0, -1):
        lin, y = layers[i], acts[i]
        N = lin.out_features
        if g.shape[1] != N:
            g = dg = ops.copy_cols_out(g, gcol, N)
        else:
            dg = torch.empty_like(g)    # d2 belongs to every feature of the aggregation
        db = _grad_buf(lin.bias)
        if N % 4 == 0:
            ops.act_bwd_bias(g, y, db, 1, out=dg)
        else:
            # the ReLU mask is element-wise: the kernel takes the buffers as rows of four (zero-padded copies where tokens * width
            # is no multiple of 4); the column sum as a product with ones
            n = g.numel()
            if n % 4 == 0:
                ops.act_bwd_bias(g.view(-1, 4), y.view(-1, 4), None, 1, out=dg.view(-1, 4))
            else:
                flat = torch.zeros((3, (n + 3) // 4, 4), device=g.device, dtype=torch.float32)
                flat[0].view(-1)[:n] = g.reshape(-1)
                flat[1].view(-1)[:n] = y.reshape(-1)
                ops.act_bwd_bias(flat[0], flat[1], None, 1, out=flat[2])
                dg = flat[2].view(-1)[:n].view(g.shape)
            ones = torch.ones((dg.shape[0], 1), device=dg.device, dtype=torch.float32)
            ops.gemm(dg, ones, True, False, accumulate=True, out=db.view(N, 1))
        ops.gemm_wgrad(dg, acts[i - 1], _grad_buf(lin.weight))
        g, gcol = ops.gemm(dg, lin.weight.detach(), False, False), 0
    lin = layers[0]
    ops.cont_proj_bwd_(g, gcol, rec["xs"], rec["flags"], lin.weight.detach(), lin.bias.detach(), _grad_buf(lin.weight),
                       _grad_buf(lin.bias))


class PretrainedEmbeddingFeatures(nn.Module):
    """Drop-in for tr.PretrainedEmbeddingFeatures (features/embedding.py:599-740): frozen text / image vectors of the items
    (or of the session), optionally projected (`projection.<feature>`, torch.nn.Linear with its default init) and normalised
    (`post.feature_layer_norm.<feature>`).

      features                names of the pretrained features
      input_dims              {name: E}, the width of each feature's vectors (the reference learns it at build time from the
                              schema's shapes; here it is a constructor argument, an int serving every feature)
      pretrained_output_dims  None, an int (every feature is projected to it) or a dict (only the named ones are)
      normalizer              None, "layer-norm" or a TabularLayerNorm

    Every feature has two forms.  DENSE, the reference's wire form: inputs[name] is a float [B, L, E] (or [B, E]) tensor, projected
    by the general GEMM and the LayerNorm kernels.  DEVICE-RESIDENT: `attach_table(name, weight [V, E], key=None)` packs the frozen
    table once into an fp16 image (ops.pack_item_table) kept as a non-persistent buffer -- it follows .to(device) and is not in the
    state_dict --, and the feature is computed from the ids inputs[key] (default: the item-id column) by the fused gather +
    projection kernel (csrc/pretrained_proj.hip); inputs[name] need not exist.  The table's values are then its fp16 roundings,
    as under the reference's autocast; there is no gradient for the table in either form."""

    def __init__(self, features, input_dims, pretrained_output_dims=None, sequence_combiner=None, pre=None, post=None,
                 aggregation=None, normalizer=None, schema=None):
        super().__init__()
        if sequence_combiner is not None:
            raise NotImplementedError("sequence_combiner on pretrained embeddings is off the hot path")
        if pre is not None or post is not None or aggregation is not None:
            raise NotImplementedError("pre / post / aggregation on PretrainedEmbeddingFeatures other than `normalizer` are off "
                                      "the hot path")
        self.features = list(features)
        self.schema = schema
        self.pretrained_output_dims = pretrained_output_dims
        self.sequence_combiner = None
        if isinstance(input_dims, int):
            input_dims = {n: input_dims for n in self.features}
        missing = [n for n in self.features if n not in input_dims]
        if missing:
            raise ValueError(f"PretrainedEmbeddingFeatures: no input width for {missing}")
        self.input_dims = {n: int(input_dims[n]) for n in self.features}
        if isinstance(pretrained_output_dims, dict):
            unknown = [n for n in pretrained_output_dims if n not in self.features]
            if unknown:
                raise ValueError(f"pretrained_output_dims names unknown features: {unknown}")
            out = {n: int(d) for n, d in pretrained_output_dims.items()}
        elif pretrained_output_dims:
            out = {n: int(pretrained_output_dims) for n in self.features}
        else:
            out = {}
        if out:
            self.projection = nn.ModuleDict({n: _Linear(self.input_dims[n], out[n]) for n in self.features if n in out})
        self._out_dims = {n: out.get(n, self.input_dims[n]) for n in self.features}
        if isinstance(normalizer, str):
            if normalizer != "layer-norm":
                raise NotImplementedError(f"normalizer {normalizer!r}: only 'layer-norm' is on the hot path")
            self.post = TabularLayerNorm(self._out_dims)        # width-1 features are skipped, as in the reference
        elif isinstance(normalizer, TabularLayerNorm):
            self.post = normalizer.build(self._out_dims)
        elif normalizer is None:
            self.post = None
        else:
            raise NotImplementedError("normalizer must be None, 'layer-norm' or a TabularLayerNorm")
        self.embedding_tables = nn.ModuleDict()     # no trainable tables (TabularSequenceFeatures._apply_pre walks this name)
        self._keys = {}

    @classmethod
    def from_schema(cls, schema, tags=None, pretrained_output_dims=None, sequence_combiner=None, normalizer=None, pre=None,
                    post=None, aggregation=None, input_dims=None, **kwargs):
        """features/embedding.py:670-695; the width of a column is input_dims[name], else the column's `embedding_dim`"""
        if tags:
            schema = schema.select_by_tag(tags)
        names = schema.column_names
        if not names:
            return None
        dims = dict(input_dims or {}) if not isinstance(input_dims, int) else {n: input_dims for n in names}
        for c in schema.feature:
            if c.name not in dims and getattr(c, "embedding_dim", None):
                dims[c.name] = int(c.embedding_dim)
        return cls(names, dims, pretrained_output_dims=pretrained_output_dims, sequence_combiner=sequence_combiner, pre=pre,
                   post=post, aggregation=aggregation, normalizer=normalizer, schema=schema)

    # ------------------------------------------------------------------ device-resident tables
    @staticmethod
    def _image_name(name):
        return "_image_" + name

    def attach_table(self, name, weight, key=None):
        """keeps the frozen table weight [V, E] of feature `name` on the device as an fp16 image; the feature is then looked up
        by inputs[key] (None: the item-id column of the block this module is merged into)"""
        if name not in self.features:
            raise KeyError(f"attach_table: {name!r} is not one of {self.features}")
        if not hasattr(self, "projection") or name not in self.projection:
            raise ValueError(f"attach_table: the device-resident form of {name!r} is gather + projection in one kernel and needs "
                             f"a projection for it: name it in pretrained_output_dims")
        if weight.dim() != 2 or weight.shape[1] != self.input_dims[name]:
            raise ValueError(f"attach_table: {name!r} takes a [V, {self.input_dims[name]}] table, got {tuple(weight.shape)}")
        image = ops.pack_item_table(weight.detach().float().contiguous(), "fp16")
        self.detach_table(name)
        # the buffer is the whole padded image [V, ld]: a copy to another device keeps the aligned row pitch
        ld = image.stride(0) if image.shape[0] > 1 else ops.image_ld(image.shape[1])
        self.register_buffer(self._image_name(name), torch.as_strided(image, (image.shape[0], ld), (ld, 1)), persistent=False)
        self._keys[name] = key
        return self

    def detach_table(self, name):
        if self._image_name(name) in self._buffers:
            del self._buffers[self._image_name(name)]
        self._keys.pop(name, None)
        return self

    def table_image(self, name):
        """the attached fp16 image of `name` as its [V, E] view, or None"""
        buf = self._buffers.get(self._image_name(name))
        return None if buf is None else buf[:, :self.input_dims[name]]

    def table_key(self, name):
        return self._keys.get(name)

    def output_dim(self, name):
        return self._out_dims[name]

    def layer_norm(self, name):
        if self.post is None or name not in self.post.feature_layer_norm:
            return None
        return self.post.feature_layer_norm[name]

    def forward_output_size(self, input_sizes=None):
        out = {}
        for n in self.features:
            lead = list(input_sizes[n][:-1]) if input_sizes and n in input_sizes else [-1]
            out[n] = torch.Size(lead + [self._out_dims[n]])
        return out


_POST_SALT = 4
_post_seed_value = None


def post_seed():
    """Philox key of the TabularDropout masks: rng.default_seed(_POST_SALT), resolved at the first draw"""
    global _post_seed_value
    if _post_seed_value is None:
        from .rng import default_seed

        _post_seed_value = default_seed(_POST_SALT)
    return _post_seed_value


def set_post_seed(value):
    """restores the TabularDropout key (rng.set_rng_state); None re-resolves it at the next draw"""
    global _post_seed_value
    _post_seed_value = None if value is None else int(value) & 0x7FFFFFFFFFFFFFFF


def _post_fwd(owner, post, name, fidx, e2d, step):
    """Applies the module's post transformations to one feature's rows e2d [rows, D].
    Dropout directly followed by the feature's LayerNorm runs as one fused launch.
    -> (rows after post, records for _post_bwd)"""
    saved = []
    mods = list(post)
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, TabularDropout):
            p = m.dropout_rate if owner.training else 0.0
            ctr = ops.dropout_ctr_hi(step, 0xFE, fidx * 8 + i)
            nxt = mods[i + 1] if i + 1 < len(mods) else None
            if isinstance(nxt, TabularLayerNorm) and name in nxt.feature_layer_norm:
                ln = nxt.feature_layer_norm[name]
                drop = (p, post_seed(), ctr) if p > 0 else ops.NO_DROP
                y, mean, rstd = ops.add_layernorm_fwd(e2d, None, ln.weight.detach(), ln.bias.detach(), ln.eps, drop)
                saved.append(("ln", e2d, mean, rstd, ln, drop))
                e2d = y
                i += 2
                continue
            if p > 0:
                e2d = ops.dropout(e2d, p, post_seed(), ctr).view(e2d.shape)
                saved.append(("drop", p, ctr))
        elif name in m.feature_layer_norm:
            ln = m.feature_layer_norm[name]
            y, mean, rstd = ops.add_layernorm_fwd(e2d, None, ln.weight.detach(), ln.bias.detach(), ln.eps)
            saved.append(("ln", e2d, mean, rstd, ln, ops.NO_DROP))
            e2d = y
        i += 1
    return e2d, saved


def _post_bwd(saved, dy):
    for rec in reversed(saved):
        if rec[0] == "drop":
            dy = ops.dropout(dy, rec[1], post_seed(), rec[2]).view(dy.shape)
        else:
            _, a, mean, rstd, ln, drop = rec
            r = ops.add_layernorm_bwd(a, None, ln.weight.detach(), mean, rstd, dy, _grad_buf(ln.weight),
                                      _grad_buf(ln.bias), drop=drop)
            dy = r[1] if drop[0] > 0 else r
    return dy


def _pretrained_fwd(mod, pt, name, inputs, B, L, col, dim, err, save):
    """one pretrained feature's rows -> (feature dict for ops.seq_features_fwd, record for _pretrained_bwd)"""
    lin = pt.projection[name] if hasattr(pt, "projection") and name in pt.projection else None
    ln = pt.layer_norm(name)
    image = pt.table_image(name)
    if image is not None:
        key = pt.table_key(name) or mod.categorical_module.item_id
        ids = inputs[key].contiguous()
        per_session = ids.ndim == 1
        rows, xhat, rstd = ops.pretrained_proj_fwd(
            image, ids, lin.weight.detach(), lin.bias.detach(), None if ln is None else ln.weight.detach(),
            None if ln is None else ln.bias.detach(), 1e-5 if ln is None else ln.eps, err_flag=err,
            save=save)
        rec = dict(form="image", image=image, ids=ids, xhat=xhat, rstd=rstd, lin=lin, ln=ln, per_session=per_session)
    else:
        if name not in inputs:
            raise KeyError(f"pretrained feature {name!r}: no inputs[{name!r}] and no attached table (attach_table)")
        x = inputs[name]
        if x.ndim not in (2, 3) or x.shape[-1] != pt.input_dims[name]:
            raise ValueError(f"pretrained feature {name!r}: expected [B, L, {pt.input_dims[name]}] or [B, {pt.input_dims[name]}], "
                             f"got {tuple(x.shape)}")
        per_session = x.ndim == 2
        x2 = x.contiguous().float().view(-1, x.shape[-1])
        rows = z = x2
        mean = rstd = None
        if lin is not None:
            rows = z = ops.gemm(x2, lin.weight.detach(), False, True, bias=lin.bias.detach(), epilogue=ops.EPI_BIAS)
        if ln is not None:
            rows, mean, rstd = ops.add_layernorm_fwd(z, None, ln.weight.detach(), ln.bias.detach(), ln.eps)
        rec = dict(form="dense", x=x2, z=z, mean=mean, rstd=rstd, lin=lin, ln=ln, per_session=per_session)
    rec["feat"] = dict(kind=3 if per_session else 1, input=rows, table=None, dim=dim, col=col)
    return rec["feat"], rec


def _pretrained_bwd(rec, d2, col, dim, B, L):
    """parameter gradients of one pretrained feature from its columns of the aggregate's gradient d2 [B * L, W]"""
    lin, ln = rec["lin"], rec["ln"]
    if lin is None and ln is None:
        return      # a pass-through column block
    if rec["per_session"]:      # broadcast over L: the gradient is the sum over the sequence
        g, gcol = ops.seq_sum_cols(d2, col, dim, B, L), 0
    else:
        g, gcol = d2, col
    if rec["form"] == "image":
        ops.pretrained_proj_bwd(g, rec["image"], rec["ids"], None if ln is None else ln.weight.detach(), rec["xhat"], rec["rstd"],
                                _grad_buf(lin.weight), _grad_buf(lin.bias), None if ln is None else _grad_buf(ln.weight),
                                None if ln is None else _grad_buf(ln.bias), col=gcol)
        return
    if g.shape[1] != dim:
        g = ops.copy_cols_out(g, col, dim)
    if ln is not None:
        g = ops.add_layernorm_bwd(rec["z"], None, ln.weight.detach(), rec["mean"], rec["rstd"], g, _grad_buf(ln.weight),
                                  _grad_buf(ln.bias))
    if lin is not None:
        db = _grad_buf(lin.bias)
        if dim % 4 == 0:
            ops.colsum_(g, db)
        else:
            ones = torch.ones((g.shape[0], 1), device=g.device, dtype=torch.float32)
            ops.gemm(g, ones, True, False, accumulate=True, out=db.view(dim, 1))
        ops.gemm_wgrad(g, rec["x"], _grad_buf(lin.weight))


class _SeqFeaturesFn(torch.autograd.Function):
    """gather (+soft embeddings) -> aggregate -> [ReLU projection] -> masking, one autograd node.
    Parameter gradients are accumulated straight into `.grad` (flat-buffer friendly)."""

    @staticmethod
    def forward(ctx, anchor, mod, inputs, training, testing):
        ctx.carrier = bool(mod.__dict__.get("_t4r_carrier_on", False))      # anchor = the GradCarrier's one-float output
        cat, cont, pt = mod.categorical_module, mod.continuous_module, mod.pretrained_module
        names = mod._feature_order
        item_ids = inputs[cat.item_id].contiguous()
        B, L = item_ids.shape
        masking = mod._masking
        mask_mode, mask, L_out = ops.MASK_NONE, None, L
        if masking is not None:
            masking.compute_masked_targets(item_ids, training=training, testing=testing)
            mask = masking.mask_schema
            mask_mode = masking.apply_mode(training, testing)
            L_out = mask.shape[1]
        feats, soft_saved, post_saved, pt_saved = [], {}, {}, {}
        ctx.cp_saved = None
        step = mod._post_step
        for fidx, name in enumerate(names):
            col, dim = mod._cols[name], mod._dims[name]
            if name in cat.embedding_tables:
                tab = cat.embedding_tables[name].weight
                ids_f = inputs[name].contiguous()
                # a [B] id tensor is a non-sequential (context) feature: looked up once per session
                # and broadcast over L (reference: tabular/base.py:53-63)
                per_session = ids_f.ndim == 1
                f = dict(kind=2 if per_session else 0, input=ids_f, table=tab.detach(), dim=dim, col=col,
                         rows=tab.shape[0])
                if cat._post is not None:
                    # post transformations act on the feature's own rows before the aggregation: gather
                    # them densely, transform, and hand them to the aggregation as dense rows
                    Lf = 1 if per_session else L
                    e = ops.seq_features_fwd([dict(f, kind=0, col=0)], "concat", B, Lf, Lf, dim,
                                             err_flag=mod._err_flag(item_ids.device)).view(B * Lf, dim)
                    e, post_saved[name] = _post_fwd(cat, cat._post, name, fidx, e, step)
                    f = dict(kind=3 if per_session else 1, input=e, table=None, dim=dim, col=col)
                feats.append(f)
            elif pt is not None and name in pt.features:
                # (grad mode is off inside forward: whether a backward can follow is the anchor's needs_input_grad)
                f, pt_saved[name] = _pretrained_fwd(mod, pt, name, inputs, B, L, col, dim, mod._err_flag(item_ids.device),
                                                    save=ctx.needs_input_grad[0])
                feats.append(f)
            elif isinstance(cont, ContinuousProjection):
                rows, ctx.cp_saved = _cont_proj_fwd(cont, inputs, B, L)
                feats.append(dict(kind=1, input=rows, table=None, dim=dim, col=col))
            elif isinstance(cont, ContinuousFeatures):
                x = inputs[name].contiguous().float().view(B * L, 1)
                if cont._post is not None:
                    x, post_saved[name] = _post_fwd(cont, cont._post, name, fidx, x, step)
                feats.append(dict(kind=1, input=x, table=None, dim=1, col=col))
            else:
                se = cont.embedding_tables[name]
                ln = cont.post.feature_layer_norm[name] if cont.post is not None else None
                x = inputs[name].contiguous().float()
                rows = ops.soft_embedding_fwd(
                    x, se.projection_layer.weight.detach(), se.projection_layer.bias.detach(),
                    se.embedding_table.weight.detach(), None if ln is None else ln.weight.detach(),
                    None if ln is None else ln.bias.detach(), 1e-5 if ln is None else ln.eps)
                soft_saved[name] = x
                feats.append(dict(kind=1, input=rows, table=None, dim=dim, col=col))
        W = mod._agg_width
        proj = mod.projection_module
        fuse_mask = masking is not None and proj is None
        memb = masking.masked_item_embedding if masking is not None else None
        item_feat = names.index(cat.item_id) if cat.item_id in names else -1
        agg_out = ops.seq_features_fwd(
            feats, mod._aggregation, B, L, L_out, W, item_feat=item_feat,
            mask_mode=mask_mode if fuse_mask else ops.MASK_NONE, mask=mask if fuse_mask else None,
            masked_emb=memb.detach() if fuse_mask else None, err_flag=mod._err_flag(item_ids.device))
        out = agg_out
        if proj is not None:
            lin = proj[0][0]
            out = ops.gemm(agg_out.view(B * L_out, W), lin.weight.detach(), False, True,
                           bias=lin.bias.detach(), epilogue=ops.EPI_BIAS_RELU).view(B, L_out, -1)
            if masking is not None:
                ops.apply_mask_fwd_(out, mask, memb.detach(), mask_mode)
        ctx.mod, ctx.inputs, ctx.soft_saved, ctx.post_saved, ctx.pt_saved = mod, inputs, soft_saved, post_saved, pt_saved
        if mod._aggregation != "element-wise-sum-item-multi":
            for rec in pt_saved.values():
                del rec["feat"]     # only that aggregation's backward aggregates the features again
        # the sort behind the deterministic table gradient depends on the ids only: done here, in the forward
        ctx.sorted_ids = {}
        if training:
            todo = []
            for name in names:
                if name in cat.embedding_tables:
                    tab = cat.embedding_tables[name].weight
                    if tab.requires_grad and getattr(tab, "_t4r_sparse_sink", None) is None:
                        todo.append((name, inputs[name].contiguous(), tab.shape[0]))
            if len(todo) > 1 and len({t[1].numel() for t in todo}) == 1 and len(todo) <= 16:
                # every table of a multi-feature block in ONE device sort (a third of the launches: ops.sort_ids_multi)
                srt = _sort_ids_forward_multi([t[1] for t in todo], [t[2] for t in todo], cat.padding_idx)
                for (name, _i, _r), s_f in zip(todo, srt):
                    ctx.sorted_ids[name] = s_f
            else:
                for name, ids_n, rows_n in todo:
                    ctx.sorted_ids[name] = _sort_ids_forward(ids_n, rows_n, cat.padding_idx)
        ctx.mask_mode, ctx.mask, ctx.dims, ctx.post_step = mask_mode, mask, (B, L, L_out, W), step
        ctx.agg_out = agg_out if proj is not None else None
        ctx.proj_out = out if proj is not None else None
        return out

    @staticmethod
    def backward(ctx, dy):
        mod = ctx.mod
        cat, cont = mod.categorical_module, mod.continuous_module
        B, L, L_out, W = ctx.dims
        if L_out != L:
            raise RuntimeError("the MLM inference grid (L+1) is forward-only")
        masking, proj = mod._masking, mod.projection_module
        if masking is not None:     # out of place: the incoming gradient is not ours to write, and a clone is a 10 MB copy
            d = ops.apply_mask_bwd(dy, ctx.mask, _grad_buf(masking.masked_item_embedding), ctx.mask_mode)
        else:
            d = dy.contiguous().clone()
        if proj is not None:
            lin = proj[0][0]
            H = d.shape[-1]
            d2 = d.view(B * L, H)
            ops.act_bwd_bias(d2, ctx.proj_out.view(B * L, H), None if lin.bias is None else _grad_buf(lin.bias), 1)
            # the projection's weight gradient (K = tokens): split-K with the partials added in split order, not atomics --
            # it was the one order-dependent sum of a configs[2] step
            ops.gemm_wgrad(d2, ctx.agg_out.view(B * L, W), _grad_buf(lin.weight))
            d = ops.gemm(d2, lin.weight.detach(), False, False).view(B, L, W)
        names = mod._feature_order
        agg = mod._aggregation
        if agg == "element-wise-sum-item-multi":
            item = cat.item_id
            def again(n):   # the feature as the forward aggregated it (post-transformed rows are recomputed)
                if n in ctx.pt_saved:
                    return dict(ctx.pt_saved[n]["feat"], dim=W, col=0)
                if n == CONTINUOUS_PROJECTION and ctx.cp_saved is not None:
                    return dict(kind=1, input=ctx.cp_saved["acts"][-1], table=None, dim=W, col=0)
                ids_n = ctx.inputs[n].contiguous()
                tabn = cat.embedding_tables[n].weight.detach()
                f = dict(kind=2 if ids_n.ndim == 1 else 0, input=ids_n, table=tabn, dim=W, col=0, rows=tabn.shape[0])
                if n in ctx.post_saved:
                    Lf = 1 if ids_n.ndim == 1 else L
                    e = ops.seq_features_fwd([dict(f, kind=0)], "concat", B, Lf, Lf, W).view(B * Lf, W)
                    e, _ = _post_fwd(cat, cat._post, n, names.index(n), e, ctx.post_step)
                    f = dict(kind=3 if ids_n.ndim == 1 else 1, input=e, table=None, dim=W, col=0)
                return f

            f_item = [again(item)]
            f_other = [again(n) for n in names if n != item]
            e_item = ops.seq_features_fwd(f_item, "element-wise-sum", B, L, L, W)
            e_other = ops.seq_features_fwd(f_other, "element-wise-sum", B, L, L, W)
            d_item, d_other = ops.mul(d, e_other), ops.mul(d, e_item)
        for name in names:
            col, dim = mod._cols[name], mod._dims[name]
            if name in cat.embedding_tables:
                tab = cat.embedding_tables[name].weight
                if not tab.requires_grad:
                    continue
                src = d
                if agg == "element-wise-sum-item-multi":
                    src = d_item if name == cat.item_id else d_other
                ids_f = ctx.inputs[name].contiguous()
                if name in ctx.post_saved:
                    src2 = src.view(B * L, -1)
                    if ids_f.ndim == 1:     # broadcast over L: the gradient is the sum over the sequence
                        g = ops.seq_sum_cols(src2, col, dim, B, L)
                    else:
                        g = ops.copy_cols_out(src2, col, dim) if src2.shape[1] != dim else src2
                    g = _post_bwd(ctx.post_saved[name], g)
                    _table_scatter(ctx, name, g, ids_f, tab, 0, dim, cat.padding_idx)
                else:
                    _table_scatter(ctx, name, src.view(-1, src.shape[-1]), ids_f, tab, col, dim, cat.padding_idx)
            elif name in ctx.pt_saved:
                src = d_other if agg == "element-wise-sum-item-multi" else d
                _pretrained_bwd(ctx.pt_saved[name], src.view(B * L, -1), col, dim, B, L)
            elif isinstance(cont, ContinuousProjection):
                src = d_other if agg == "element-wise-sum-item-multi" else d
                _cont_proj_bwd(cont, ctx.cp_saved, src.view(B * L, -1), col)
            elif isinstance(cont, ContinuousFeatures):
                continue    # no parameters behind a pass-through column
            else:
                se = cont.embedding_tables[name]
                ln = cont.post.feature_layer_norm[name] if cont.post is not None else None
                ops.soft_embedding_bwd(
                    d, ctx.soft_saved[name], se.projection_layer.weight.detach(),
                    se.projection_layer.bias.detach(), se.embedding_table.weight.detach(),
                    None if ln is None else ln.weight.detach(), _grad_buf(se.projection_layer.weight),
                    _grad_buf(se.projection_layer.bias), _grad_buf(se.embedding_table.weight),
                    None if ln is None else _grad_buf(ln.weight), None if ln is None else _grad_buf(ln.bias),
                    col, 1e-5 if ln is None else ln.eps)
        # the anchor's slot: a defined (zero) gradient for the GradCarrier's output, so that its node -- the last of the
        # backward pass -- runs and hands the carried parameter gradients to autograd
        return (torch.zeros(1, device=dy.device) if ctx.carrier else None), None, None, None, None


class TabularSequenceFeatures(nn.Module):
    """Drop-in for tr.TabularSequenceFeatures on the hot path (features/sequence.py:97-296).

    forward(inputs: Dict[str, Tensor[B, L]], training=False, testing=False) -> Tensor[B, L(+1), H]
    """

    def __init__(self, categorical_module: SequenceEmbeddingFeatures,
                 continuous_module: Optional[SoftEmbeddingFeatures] = None, aggregation: str = "concat",
                 projection_dim: Optional[int] = None, masking: Optional[MaskSequence] = None,
                 schema=None, max_sequence_length: Optional[int] = None,
                 pretrained_embedding_module: Optional[PretrainedEmbeddingFeatures] = None):
        super().__init__()
        if aggregation not in ops.AGG:
            raise ValueError(f"aggregation must be one of {sorted(ops.AGG)}")
        self.schema = schema
        self.max_sequence_length = max_sequence_length
        mods = {}
        if continuous_module is not None:
            mods["continuous_module"] = continuous_module
        mods["categorical_module"] = categorical_module
        if pretrained_embedding_module is not None:
            mods["pretrained_embedding_module"] = pretrained_embedding_module
        self.to_merge = nn.ModuleDict(mods)
        self._aggregation = aggregation
        self.projection_module = None
        self._layout()
        if projection_dim:
            # MLPBlock([d_output]) -> SequentialBlock(DenseBlock(Linear, ReLU)) (block/mlp.py:68-143)
            self.projection_module = nn.Sequential(nn.Sequential(_Linear(self._agg_width, projection_dim)))
        self._masking = None
        self.set_masking(masking)
        self._err = None
        self._post_step = 0     # Philox stream position of the post-dropout / swap-noise draws

    def _layout(self):
        """names, widths and columns of the features the aggregation sees, from the modules in `to_merge`"""
        categorical_module, continuous_module = self.categorical_module, self.continuous_module
        pretrained_embedding_module, aggregation = self.pretrained_module, self._aggregation
        dims = {n: t.embedding_dim for n, t in categorical_module.embedding_tables.items()}
        if isinstance(continuous_module, ContinuousProjection):
            dims[CONTINUOUS_PROJECTION] = continuous_module.output_dim
        elif isinstance(continuous_module, ContinuousFeatures):
            dims.update({n: 1 for n in continuous_module.names})
        elif continuous_module is not None:
            dims.update({n: s.embedding_table.embedding_dim for n, s in continuous_module.embedding_tables.items()})
        if pretrained_embedding_module is not None:
            clash = [n for n in pretrained_embedding_module.features if n in dims]
            if clash:
                raise ValueError(f"pretrained features share names with other features: {clash}")
            dims.update({n: pretrained_embedding_module.output_dim(n) for n in pretrained_embedding_module.features})
        # ConcatFeatures order = sorted(feature names) (tabular/aggregation.py:43)
        self._feature_order = sorted(dims)
        self._dims = dims
        if aggregation == "concat":
            off, cols = 0, {}
            for n in self._feature_order:
                cols[n] = off
                off += dims[n]
            self._cols, self._agg_width = cols, off
        else:
            if len(set(dims.values())) != 1:
                raise ValueError(f"All features must have the same dimension for element-wise aggregation: {dims}")
            self._cols, self._agg_width = {n: 0 for n in dims}, next(iter(dims.values()))

    # ------------------------------------------------------------------ reference attribute contract
    @property
    def categorical_module(self):
        return self.to_merge["categorical_module"]

    @property
    def continuous_module(self):
        return self.to_merge["continuous_module"] if "continuous_module" in self.to_merge else None

    @property
    def pretrained_module(self):
        return self.to_merge["pretrained_embedding_module"] if "pretrained_embedding_module" in self.to_merge else None

    @property
    def masking(self):
        return self._masking

    def set_masking(self, value):
        self._masking = value

    @property
    def item_id(self):
        return self.categorical_module.item_id

    @property
    def item_embedding_table(self):
        return self.categorical_module.item_embedding_table

    @property
    def aggregation(self):
        return self._aggregation

    def output_size(self, input_size=None):
        H = self.projection_module[0][0].out_features if self.projection_module is not None else self._agg_width
        return torch.Size([-1, self.max_sequence_length or -1, H])

    forward_output_size = output_size

    def _err_flag(self, device):
        if self._err is None or self._err.device != device:
            self._err = torch.zeros(1, dtype=torch.int32, device=device)
        return self._err

    def check_ids(self):
        """Raises if any lookup id was out of range since the last check (device flag, syncs)."""
        if self._err is not None and int(self._err.item()) != 0:
            self._err.zero_()
            raise IndexError("embedding lookup id out of range")

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_schema(cls, schema, continuous_tags=(Tags.CONTINUOUS,), categorical_tags=(Tags.CATEGORICAL,),
                    pretrained_embeddings_tags=(Tags.EMBEDDING,), aggregation=None, max_sequence_length=None, continuous_soft_embeddings=False,
                    d_output=None, masking=None, embedding_dims=None, embedding_dim_default=64,
                    soft_embedding_cardinalities=None, soft_embedding_cardinality_default=10,
                    soft_embedding_dims=None, soft_embedding_dim_default=8, layer_norm=True,
                    projection=None, continuous_projection=None, pre=None, post=None, pretrained_output_dims=None,
                    normalizer=None, pretrained_input_dims=None, **kwargs):
        """Same keyword surface as the reference (features/sequence.py:140-229,
        features/embedding.py:103-221, :313-410) for the arguments the hot path uses."""
        if projection is not None:
            raise NotImplementedError("projection (a custom block): only d_output (ReLU MLP) and continuous_projection are on "
                                      "the hot path")
        if continuous_projection is not None and continuous_soft_embeddings:
            raise NotImplementedError("continuous_projection with continuous_soft_embeddings=True (soft embeddings fed into the "
                                      "projection) is off the hot path")
        cat_schema = schema.select_by_tag(list(categorical_tags))
        cards = categorical_cardinalities(cat_schema)
        if not cards:
            raise ValueError("a categorical_module including an item_id column is required")
        item_cols = schema.select_by_tag(Tags.ITEM_ID).column_names
        item_id = item_cols[0] if item_cols else None
        embedding_dims = embedding_dims or {}
        tables = {n: (v, embedding_dims.get(n, embedding_dim_default)) for n, v in cards.items()}
        # pre / post reach every feature module through **kwargs in the reference
        # (features/tabular.py:150-185); soft embeddings replace `post` by their LayerNorm
        cat = SequenceEmbeddingFeatures(tables, item_id=item_id, pre=pre, post=post)
        cont = None
        pt = None
        if pretrained_embeddings_tags:
            tags = pretrained_embeddings_tags
            pt = PretrainedEmbeddingFeatures.from_schema(
                schema, tags=list(tags) if isinstance(tags, (list, tuple, set)) else [tags],
                pretrained_output_dims=pretrained_output_dims, normalizer=normalizer, input_dims=pretrained_input_dims)
        if pt is not None and (pre is not None or post is not None):
            raise NotImplementedError("pre / post transformations on pretrained embeddings other than `normalizer` are off the "
                                      "hot path")
        pt_names = set(pt.features) if pt is not None else set()
        cont_names = [c for c in schema.select_by_tag(list(continuous_tags)).column_names
                      if c not in cards and c not in pt_names]
        if cont_names and not continuous_soft_embeddings:
            cont = ContinuousFeatures(cont_names, pre=pre, post=post)     # features/continuous.py:60-63
        elif cont_names:
            sc, sd = soft_embedding_cardinalities or {}, soft_embedding_dims or {}
            cont = SoftEmbeddingFeatures(
                {n: (sc.get(n, soft_embedding_cardinality_default), sd.get(n, soft_embedding_dim_default))
                 for n in cont_names}, layer_norm=layer_norm, pre=pre, post=None if layer_norm else post)
        if continuous_projection is not None:
            if cont is None:
                raise ValueError("continuous_projection: the schema has no continuous column to project")
            cont = ContinuousProjection(cont, continuous_projection)
        if (masking or d_output) and not aggregation:
            aggregation = "concat"
        out = cls(cat, cont, aggregation or "concat", d_output, None, schema, max_sequence_length, pretrained_embedding_module=pt)
        hidden = out.output_size()[-1]
        if masking is not None and item_id is None:
            raise ValueError("For masking a categorical_module is required including an item_id.")
        out.set_masking(parse_masking(masking, hidden, **kwargs))
        return out

    def project_continuous_features(self, mlp_layers_dims):
        """features/tabular.py:90-117: puts ReLU MLP layers over the concatenated continuous columns; they then enter the
        aggregation as the one feature `continuous_projection`.  Returns self."""
        cont = self.continuous_module
        if cont is None:
            raise ValueError("project_continuous_features (continuous_projection): there is no continuous module to project")
        if isinstance(cont, ContinuousProjection):
            raise ValueError("project_continuous_features (continuous_projection): the continuous module is projected already")
        width = self._agg_width
        device = self.item_embedding_table.weight.device         # a block that was moved already gets its new layers there
        self.to_merge["continuous_module"] = ContinuousProjection(cont, mlp_layers_dims).to(device)
        try:
            self._layout()
        except ValueError:
            self.to_merge["continuous_module"] = cont
            self._layout()
            raise
        if self._agg_width != width:
            if self.projection_module is not None:
                lin = self.projection_module[0][0]
                self.projection_module = nn.Sequential(nn.Sequential(_Linear(self._agg_width, lin.out_features))).to(device)
            elif self._masking is not None:
                self.to_merge["continuous_module"] = cont
                self._layout()
                raise ValueError("project_continuous_features (continuous_projection) changes the width the masking module was "
                                 "built for: project before the masking is set")
        return self

    # ------------------------------------------------------------------ forward
    def _apply_pre(self, inputs):
        """StochasticSwapNoise of each feature module on its own features (TabularModule.__call__ runs
        `pre` before forward, tabular/base.py:389); the padding mask comes from the ORIGINAL item ids."""
        active = {}
        out = inputs
        for mi, (mname, m) in enumerate(self.to_merge.items()):
            ssn = getattr(m, "_pre", None)
            if ssn is None or not ssn.training:
                continue
            if out is inputs:
                out = dict(inputs)
                item_ids = inputs[self.categorical_module.item_id].contiguous()
            names = list(m.names) if isinstance(m, (ContinuousFeatures, ContinuousProjection)) else list(m.embedding_tables.keys())
            out.update(ssn.augment_module(inputs, [n for n in names if n in inputs], item_ids, mname, mi))
            active[id(ssn)] = ssn
        for ssn in active.values():     # one stream position per forward, also when modules share the object
            ssn.next_step()
        return out

    def forward(self, inputs, training=False, testing=False, **kwargs):
        cat = self.categorical_module
        inputs = self._apply_pre(inputs)
        if cat.item_id:
            cat.item_seq = cat.item_ids(inputs)  # stateful, as the reference (embedding.py:242-245); after `pre`
        if self.training:
            self._post_step += 1
        anchor = cat.item_embedding_table.weight
        carried = self.__dict__.get("_t4r_carrier_params")
        object.__setattr__(self, "_t4r_carrier_on", False)
        if carried and torch.is_grad_enabled() and (training or self.training):
            from .masking import GradCarrier

            GradCarrier.release(carried)                 # leftovers of a forward whose backward never ran
            anchor = GradCarrier.apply(carried, *carried)      # autograd-visible parameter gradients (masking.GradCarrier)
            object.__setattr__(self, "_t4r_carrier_on", True)
        return _SeqFeaturesFn.apply(anchor, self, inputs, training, testing)
