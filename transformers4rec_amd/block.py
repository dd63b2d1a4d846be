"""MLPBlock: host-side mirror of transformers4rec/torch/block/mlp.py for the hot path -- the dense stack the reference's
examples put between the input block and the transformer,

    body = SequentialBlock(input_module, MLPBlock([d_model]), TransformerBlock(...))      ->      Model(..., mlp_block=MLPBlock([d_model]))

Same constructor arguments; `.build(input_shape)` gives the built stack with the reference's parameter names `<i>.0.weight` and
`<i>.0.bias` (layer i is a DenseBlock whose member 0 is the Linear) initialised as torch.nn.Linear initialises.  Arithmetic:
csrc/mlp_block.hip (include/t4r_hip_mlpblock.h) -- the whole stack is one launch forward and at most three backward; in evaluation
and inference the intermediate activations never reach memory.

On the HIP path: activation torch.nn.ReLU or None, with or without bias, dropout; 1 .. 4 layers, input width <= 1024, layer widths
<= 512.  Everything else (another activation, normalization, filter_features, wider or deeper stacks) raises NotImplementedError.
"""
import torch
from torch import nn

from . import ops
from .features import _Linear
from .masking import _grad_buf
from .rng import SeedMixin


class _MLPStackFn(torch.autograd.Function):
    """x [..., K0] -> a_{n-1} [..., N_{n-1}]; the backward returns d x and ACCUMULATES the parameter gradients into
    masking._grad_buf (the package's convention; a frozen parameter gets a scratch buffer) and returns None for them."""

    @staticmethod
    def forward(ctx, x, anchor, stack, drop, save):
        """save: a backward may follow (grad mode was on at the call): every a_i is stored; else only the last one is written"""
        x = x.detach().contiguous()
        Ws, bs = stack._weights(), stack._biases()
        if not save:
            return ops.mlp_stack_fwd(x, Ws, bs, stack.relu, drop)
        acts = ops.mlp_stack_fwd(x, Ws, bs, stack.relu, drop, save_acts=True)
        ctx.stack, ctx.drop = stack, drop
        ctx.save_for_backward(x, *acts)
        return acts[-1]

    @staticmethod
    def backward(ctx, dout):
        x, *acts = ctx.saved_tensors
        stack = ctx.stack
        lins = [dense[0] for dense in stack]
        d_w = [_grad_buf(lin.weight) for lin in lins]
        d_b = [_grad_buf(lin.bias) for lin in lins] if stack.use_bias else None
        dx = ops.mlp_stack_bwd_(dout.contiguous(), x, stack._weights(), acts, stack.relu, ctx.drop, d_w, d_b,
                                want_dx=ctx.needs_input_grad[0])
        return dx, None, None, None, None


class DenseBlock(nn.ModuleList):
    """one layer of the stack: member 0 is the Linear (the reference's DenseBlock, block/mlp.py:90-150, holds the activation and
    the dropout as further members without parameters; here they are the stack's kernel arguments)"""

    def __init__(self, in_features, out_features, use_bias=True):
        super().__init__([_Linear(in_features, out_features, bias=use_bias)])
        self._output_size = out_features

    def _get_name(self):
        return "DenseBlock"

    def forward_output_size(self, input_size):
        return torch.Size(list(input_size[:-1]) + [self._output_size])


class MLPStack(SeedMixin, nn.ModuleList):
    """The built MLPBlock: DenseBlocks `0 .. n-1`.  `_drop_offset` is the stream position of its dropout masks (advanced once per
    training forward; rng.get_rng_state / set_rng_state carry it), `seed` the key (rng.SeedMixin)."""
    _t4r_hip = True         # masking.hip_parameters: every parameter below this module is on the HIP path
    _seed_salt = 8

    def __init__(self, input_shape, dimensions, relu=True, use_bias=True, dropout=None):
        in_width = int(input_shape[-1])
        dims = [int(d) for d in dimensions]
        if not ops.mlp_stack_supported(in_width, dims):
            raise NotImplementedError(f"MLPBlock: the fused stack takes 1 .. {ops.MLP_MAX_LAYERS} layers, an input of 1 .. "
                                      f"{ops.MLP_MAX_K0} columns and layers of 1 .. {ops.MLP_MAX_N} (got {in_width} -> {dims})")
        super().__init__([DenseBlock(k, n, use_bias) for k, n in zip([in_width] + dims[:-1], dims)])
        self.input_size = input_shape
        self.relu, self.use_bias = bool(relu), bool(use_bias)
        self.dropout = float(dropout) if dropout else 0.0
        if not 0.0 <= self.dropout < 1.0:
            raise ValueError(f"MLPBlock: dropout must be in [0, 1), got {dropout}")
        self._drop_offset = 0

    def _weights(self):
        return [dense[0].weight.detach() for dense in self]

    def _biases(self):
        return [dense[0].bias.detach() for dense in self] if self.use_bias else None

    @property
    def in_features(self):
        return self[0][0].in_features

    @property
    def out_features(self):
        return self[-1][0].out_features

    def forward(self, x, training=None, **kwargs):
        """x [..., in_features] fp32 on the GPU -> [..., out_features].  training: default self.training; evaluation and
        dropout in (None, 0) take drop_p = 0"""
        training = self.training if training is None else training
        drop = ops.NO_DROP
        if training and self.dropout > 0:
            self._drop_offset += 1
            drop = (self.dropout, self.seed, self._drop_offset)
        return _MLPStackFn.apply(x, self[0][0].weight, self, drop, torch.is_grad_enabled())

    def _get_name(self):
        return "SequentialBlock"

    def output_size(self, input_size=None):
        return self.forward_output_size(self.input_size if input_size is None else input_size)

    def forward_output_size(self, input_size):
        return torch.Size(list(input_size[:-1]) + [self.out_features])


class MLPBlock:
    """Drop-in for transformers4rec.torch.MLPBlock (block/mlp.py:23-87): the recipe of a dense stack; `build(input_shape)` makes
    the module.  Model(..., mlp_block=MLPBlock(dims)) builds it on the input block's output size."""

    def __init__(self, dimensions, activation=torch.nn.ReLU, use_bias=True, dropout=None, normalization=None, filter_features=None):
        if isinstance(dimensions, int):
            dimensions = [dimensions]
        if activation is not None and activation is not torch.nn.ReLU:
            raise NotImplementedError(f"MLPBlock: activation {activation!r} is off the HIP hot path: the fused stack has "
                                      "torch.nn.ReLU or None.")
        if normalization:
            raise NotImplementedError("MLPBlock: normalization (batch_norm) is off the HIP hot path.")
        if filter_features:
            raise NotImplementedError("MLPBlock: filter_features selects from a dictionary of features; in the body the block "
                                      "takes the input block's one tensor, so it is not supported.")
        self.dimensions = [int(d) for d in dimensions]
        self.activation, self.use_bias, self.dropout = activation, bool(use_bias), dropout
        self.normalization, self.filter_features = None, None

    def build(self, input_shape):
        return MLPStack(input_shape, self.dimensions, relu=self.activation is not None, use_bias=self.use_bias, dropout=self.dropout)
