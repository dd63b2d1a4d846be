"""PostContextFusion: host-side mirror of transformers4rec/torch/experimental.py:22-113, the Latent Cross block that merges
context which must not go through the sequence model (features of the target item, user- or session-level features) with the
body's output right before the prediction task.

Same constructor arguments, attributes (`sequential_module`, `post_context_module`, `fusion_aggregation`, `context_projection`
-- for the two elementwise aggregations only --, `seq_length`, `last_dim`, `inputs`, `output_size()`, `forward_output_size()`)
and state_dict names (`sequential_module.{0,1}.*`, `post_context_module.*`, `context_projection.{weight,bias}`).  Arithmetic:
csrc/post_fusion.hip (include/t4r_hip_postfusion.h) -- one launch forward and at most three backward, where the reference's op
chain is four and about nine.

A 2-D context [B, C] is repeated over the L positions inside the kernels.  (The reference means to, experimental.py:85-87, but
reads `self.sequence_length` where it set `self.seq_length` and raises AttributeError; the evident intent is implemented here.)
"""
import torch
from torch import nn

from . import ops
from .features import EmbeddingFeatures, _Linear
from .masking import _grad_buf
from .model import _Body

AGGREGATIONS = ("concat", "elementwise-mul", "elementwise-sum")


def _unsupported(aggregation):
    # the reference's message (experimental.py:99-103)
    return ValueError(f"The aggregation {aggregation} is not supported, please select one of the following aggregations "
                      f"['concat', 'elementwise-mul', 'elementwise-sum']")


def context_width(module):
    """the last dimension of what `module` returns: its output_size()[-1], or the summed table widths of a concatenating
    EmbeddingFeatures"""
    size = getattr(module, "output_size", None)
    size = size() if callable(size) else None
    if size is not None and not isinstance(size, dict):
        return int(size[-1])
    if size is None and isinstance(module, EmbeddingFeatures) and module.aggregation == "concat":
        return int(sum(f.table.dim for f in module.feature_config.values()))
    raise ValueError("post_context_module must return ONE tensor (aggregation='concat') and say how wide it is: it needs an "
                     "output_size() that is a size, not a dict of sizes, or to be an EmbeddingFeatures(aggregation='concat')")


class _PostFusionFn(torch.autograd.Function):
    """(seq [B, L, D], context [B, L, C] or [B, C]) -> the fused output; the backward returns the gradients of both and
    ACCUMULATES the projection's gradients into masking._grad_buf (the package's convention); a frozen parameter gets no buffer
    (NULL)."""

    @staticmethod
    def forward(ctx, seq, context, anchor, fusion):
        lin = getattr(fusion, "context_projection", None)
        W = None if lin is None else lin.weight.detach()
        b = None if lin is None else lin.bias.detach()
        seq, context = seq.detach().contiguous(), context.detach().contiguous()
        out = ops.post_fusion_fwd(seq, context, W, b, fusion._mode)
        ctx.fusion = fusion
        ctx.save_for_backward(seq if fusion._mode == ops.FUSION_MUL else None, context)
        return out

    @staticmethod
    def backward(ctx, dout):
        seq, context = ctx.saved_tensors
        fusion = ctx.fusion
        lin = getattr(fusion, "context_projection", None)
        W = b = d_w = d_b = None
        if lin is not None:
            W, b = lin.weight.detach(), lin.bias.detach()
            d_w = _grad_buf(lin.weight) if lin.weight.requires_grad else None
            d_b = _grad_buf(lin.bias) if lin.bias.requires_grad else None
        dseq, dctx = ops.post_fusion_bwd_(dout.contiguous(), seq, context, W, b, fusion._mode, d_w, d_b,
                                          want_dseq=ctx.needs_input_grad[0], want_dctx=ctx.needs_input_grad[1])
        return dseq, dctx, None, None


class PostContextFusion(nn.Module):
    """Drop-in for transformers4rec.torch.experimental.PostContextFusion on the hot path.

    sequential_module: a model._Body, or a pair (input_features, transformer_block) that is wrapped in one.
    post_context_module: any module called as module(inputs, training=training) that returns an fp32 device tensor [B, L, C]
    (sequence-level context) or [B, C] (session-level) taking part in autograd, e.g. EmbeddingFeatures(aggregation="concat"),
    SequenceEmbeddingFeatures(aggregation="concat") or a TabularSequenceFeatures without masking."""
    _t4r_hip = True         # masking.hip_parameters: every parameter below this module is on the HIP path

    def __init__(self, sequential_module, post_context_module, fusion_aggregation="elementwise-mul"):
        super().__init__()
        if fusion_aggregation not in AGGREGATIONS:
            raise _unsupported(fusion_aggregation)
        if not isinstance(sequential_module, _Body):
            if not isinstance(sequential_module, (tuple, list)) or len(sequential_module) != 2:
                raise ValueError("sequential_module must be a body or a pair (input_features, transformer_block)")
            sequential_module = _Body(list(sequential_module))
        self.sequential_module = sequential_module
        self.post_context_module = post_context_module
        self.fusion_aggregation = fusion_aggregation
        self._mode = ops.FUSION[fusion_aggregation]
        hidden_dim = int(sequential_module[-1].transformer.config.hidden_size)
        width = context_width(post_context_module)
        if not (1 <= hidden_dim <= 1024 and 1 <= width <= 256):
            raise ValueError(f"PostContextFusion: the fused kernels take 1 <= d_model <= 1024 and a context of 1 <= C <= 256 "
                             f"columns (got d_model = {hidden_dim}, C = {width})")
        self.seq_length = sequential_module.inputs.max_sequence_length or -1
        if fusion_aggregation == "concat":
            self.last_dim = hidden_dim + width
        else:
            self.last_dim = hidden_dim
            self.context_projection = _Linear(width, hidden_dim)

    @property
    def inputs(self):
        return self.sequential_module.inputs

    def fuse(self, seq_rep, context_rep):
        """the fusion of a body output [B, L, D] and a context [B, L, C] or [B, C]"""
        lin = getattr(self, "context_projection", None)
        return _PostFusionFn.apply(seq_rep, context_rep, None if lin is None else lin.weight, self)

    def forward(self, inputs, training=False, testing=False, **kwargs):
        kwargs.pop("out_rows", None)        # every row of the body is computed: the fusion reads them
        seq_rep = self.sequential_module(inputs, training=training, testing=testing, **kwargs)
        context_rep = self.post_context_module(inputs, training=training)
        if not torch.is_tensor(context_rep) or context_rep.dim() not in (2, 3):
            raise ValueError("post_context_module must return one tensor [B, L, C] or [B, C] (aggregation='concat')")
        return self.fuse(seq_rep, context_rep.float())

    def _get_name(self):
        return "PostContextFusion"

    def output_size(self, input_size=None):
        return [-1, self.seq_length, self.last_dim]

    def forward_output_size(self, input_size):
        return torch.Size(list(input_size[:-1]) + [self.last_dim])
